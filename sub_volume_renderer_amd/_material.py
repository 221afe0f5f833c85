"""``SubVolumeMaterial`` — the parameter block of the LMIP march.

Drop-in for the reference's ``SubVolumeMaterial(gfx.VolumeMipMaterial)``
(``src/sub_volume/_material.py``): same constructor arguments and defaults, same property
names, same exception types on bad values.  The reference stores the values in a pygfx
uniform buffer; here they live in a plain dict of numpy values with the field types of that
uniform block (``_material.py:6-24``: f4 / i4 / 3xf4 / u4 / n*4xf4) and reach the device
through ``svr_set_material`` (include/svr.h) whenever ``_version`` moved.

The scalar uniforms are declared once, as data descriptors (``_Scalar``); the three
structured ones (``clim``, ``fog_color``, ``colors``) are properties with their own checks.
"""

from __future__ import annotations

import numbers

import numpy as np

# the hues pygfx-side code falls back to when no colours are given (_material.py:51-57)
_DEFAULT_HUES = (0.0, 0.25, 0.5, 0.75)


class _Scalar:
    """One scalar uniform: converts on assignment to the uniform's storage type and bumps the
    material's version so that the next draw re-sends the block."""

    def __init__(self, storage, doc, lo=None, hi=None):
        self.storage, self.lo, self.hi = storage, lo, hi
        self.__doc__ = doc

    def __set_name__(self, owner, name):
        self.field = name

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        value = obj._u[self.field]
        return float(value) if self.lo is not None else value      # clamped fields read back as python floats

    def __set__(self, obj, value):
        number = int(value) if np.issubdtype(self.storage, np.integer) else float(value)
        if self.lo is not None:
            number = min(max(number, self.lo), self.hi)
        obj._store(self.field, self.storage(number))


class SubVolumeMaterial:
    # inherited from pygfx's VolumeMipMaterial in the reference
    gamma = _Scalar(np.float32, "Exponent applied to the contrast-limited value before colouring.", -np.inf, np.inf)
    opacity = _Scalar(np.float32, "Alpha written for hit pixels (fs_main.wgsl:86), kept inside [0, 1].", 0.0, 1.0)
    # the LMIP uniforms (_material.py:60-99)
    lmip_threshold = _Scalar(np.float32, "The minimum intensity considered significant for the LMIP algorithm.")
    lmip_fall_off = _Scalar(np.float32, "The fraction of the maximum intensity that is still considered significant.")
    lmip_max_samples = _Scalar(np.int32, "How many samples are examined after the first significant one (i32 in the shader).")
    fog_density = _Scalar(np.float32, "The density of the fog effect applied to the volume.")

    def __init__(
        self,
        lmip_threshold: float,
        lmip_fall_off: float = 0.5,
        lmip_max_samples: int = 10,
        fog_density: float = 0.5,
        fog_color: tuple[float, float, float] = (0.5, 0.5, 0.5),
        colors: list[tuple[float, float, float]] | None = None,
        clim: tuple[float, float] = (0, 1),
        gamma: float = 1.0,
        opacity: float = 1.0,
    ):
        self._u = {}
        self._version = 0
        self.depth_test = True          # the reference insists on depth testing (_material.py:39-45)
        # inherited from pygfx's Material: no clipping planes unless the caller sets some
        self.clipping_planes = ()
        self.clipping_mode = "ANY"
        self.cut_planes = ()
        self.cut_mode = "ANY"
        self.render_mode = "lmip"
        self.interpolation = "nearest"
        self.weight_falloff = 0.5
        self.transfer_function = None
        self.alpha_cutoff = 0.99
        self.color_by_label = False
        self.iso_value = 0.5
        self.iso_color = (0.8, 0.8, 0.8)
        self.iso_refine = 4
        self.ambient = 0.2
        self.diffuse = 0.7
        self.specular = 0.3
        self.shininess_log2 = 5
        self.light_direction = None
        arguments = dict(clim=clim, gamma=gamma, opacity=opacity, lmip_threshold=lmip_threshold,
                         lmip_fall_off=lmip_fall_off, lmip_max_samples=lmip_max_samples, fog_density=fog_density,
                         fog_color=fog_color,
                         colors=[(h, 1.0, 1.0) for h in _DEFAULT_HUES] if colors is None else colors)
        for name, value in arguments.items():
            setattr(self, name, value)

    def _store(self, field, value):
        self._u[field] = value
        self._version += 1

    # -- clim (VolumeMipMaterial) ----------------------------------------------------------------
    @property
    def clim(self) -> tuple[float, float]:
        """The contrast limits applied before colouring (sampled_value_to_color)."""
        lo, hi = self._u["clim"]
        return float(lo), float(hi)

    @clim.setter
    def clim(self, limits) -> None:
        if not isinstance(limits, (tuple, list)) or len(limits) != 2:
            raise TypeError("Material.clim must be a 2-tuple")
        self._store("clim", np.asarray([float(v) for v in limits], np.float32))

    # -- fog colour: three numbers in [0, 1], anything else is a ValueError (_material.py:100-117) --------
    @property
    def fog_color(self) -> tuple[float, float, float]:
        """The color of the fog effect applied to the volume."""
        return tuple(self._u["fog_color"])

    @fog_color.setter
    def fog_color(self, rgb) -> None:
        components = list(rgb)
        if len(components) != 3:
            raise ValueError(f"fog_color needs exactly three components (r, g, b), got {len(components)}")
        for c in components:
            if not isinstance(c, numbers.Real):
                raise ValueError(f"fog_color components must be numbers, not {type(c).__name__}")
        packed = np.asarray(components, np.float32)
        if packed.min() < 0.0 or packed.max() > 1.0:
            raise ValueError("fog_color components must lie in [0, 1]")
        self._store("fog_color", packed)

    # -- clipping planes (pygfx Material; the shader includes pygfx.clipping_planes.wgsl, fs_main.wgsl:8) ----
    MAX_CLIPPING_PLANES = 8

    @property
    def clipping_planes(self) -> list[tuple[float, float, float, float]]:
        """World-space planes (a, b, c, d).  The draw skips a pixel whose ray leaves the volume's box at a
        point p with ``dot(p, abc) < d`` for ANY plane (``clipping_mode == "ANY"``) or for ALL of them."""
        return [tuple(map(float, row)) for row in self._u["clipping_planes"]]

    @clipping_planes.setter
    def clipping_planes(self, planes) -> None:
        rows = []
        for plane in planes:
            if isinstance(plane, (str, bytes)) or len(plane) != 4:
                raise TypeError(f"Each clipping plane must be an abcd tuple, not {plane}")
            rows.append([float(v) for v in plane])
        if len(rows) > self.MAX_CLIPPING_PLANES:
            raise ValueError(f"at most {self.MAX_CLIPPING_PLANES} clipping planes are supported")
        self._store("clipping_planes", np.asarray(rows, np.float32).reshape(-1, 4))

    @property
    def clipping_mode(self) -> str:
        """"ANY": a point is clipped if it is behind any plane; "ALL": only if it is behind all of them."""
        return self._u["clipping_mode"]

    @clipping_mode.setter
    def clipping_mode(self, mode) -> None:
        mode = str(mode).upper()
        if mode not in ("ANY", "ALL"):
            raise ValueError(f"Unexpected clipping_mode: {mode}")
        self._store("clipping_mode", mode)

    # -- cut planes (svr_set_cut_planes): the cut-away view of the "composite" and "iso" modes ---------------------
    MAX_CUT_PLANES = 8

    @property
    def cut_planes(self) -> list[tuple[float, float, float, float]]:
        """World-space planes (a, b, c, d) that open the volume up in the "composite" and "iso" render modes: a point
        p with ``dot(p, abc) < d`` is behind a plane, and the part of the volume behind ANY plane (``cut_mode ==
        "ANY"``: what stays is the intersection of the half-spaces) or behind ALL of them ("ALL": a convex wedge is
        removed) is not sampled.  Unlike ``clipping_planes``, which drop whole pixels, these shorten rays; in "iso"
        mode the cut faces are flat, lit caps (``svr_set_cut_planes`` in ``include/svr.h``).  The march ("lmip",
        "mip", "weighted_average") knows no cuts: ``SubVolume.render`` refuses those modes while planes are set."""
        return [tuple(map(float, row)) for row in self._u["cut_planes"]]

    @cut_planes.setter
    def cut_planes(self, planes) -> None:
        rows = []
        for plane in planes:
            if isinstance(plane, (str, bytes)) or len(plane) != 4:
                raise TypeError(f"Each cut plane must be an abcd tuple, not {plane}")
            rows.append([float(v) for v in plane])
        if len(rows) > self.MAX_CUT_PLANES:
            raise ValueError(f"at most {self.MAX_CUT_PLANES} cut planes are supported")
        with np.errstate(over="ignore"):
            table = np.asarray(rows, np.float32).reshape(-1, 4)
            if not np.all(np.isfinite(table)):
                raise ValueError("every component of a cut plane must be finite (as float32)")
            length = np.sqrt((table[:, 0] * table[:, 0] + table[:, 1] * table[:, 1]) + table[:, 2] * table[:, 2])
        if not np.all((length > 0) & np.isfinite(length)):
            raise ValueError("a cut plane's normal (a, b, c) must have a finite, non-zero length (as float32)")
        self._store("cut_planes", table)

    @property
    def cut_mode(self) -> str:
        """"ANY": a point is cut away if it is behind any cut plane; "ALL": only if it is behind all of them."""
        return self._u["cut_mode"]

    @cut_mode.setter
    def cut_mode(self, mode) -> None:
        mode = str(mode).upper()
        if mode not in ("ANY", "ALL"):
            raise ValueError(f"Unexpected cut_mode: {mode}")
        self._store("cut_mode", mode)

    # -- render mode: the swappable raycast the reference wishes for (FUTURE.md:97-120) -------------------------
    RENDER_MODES = ("lmip", "mip", "weighted_average", "composite", "iso")

    @property
    def render_mode(self) -> str:
        """"lmip" (the reference's raycast.wgsl) or "mip": the maximum over the WHOLE ray, first occurrence —
        what pygfx's own ``VolumeMipMaterial`` raycast selects (without its sub-step refinement).  MIP is the
        LMIP state machine with every sample significant, no fall-off and no sample limit, so it runs on the
        same kernel: the draw sends threshold = -inf, fall_off = 0, max_samples = 2**31 - 1 and leaves the
        ``lmip_*`` properties untouched.

        "weighted_average": the mode FUTURE.md:97-109 wishes for ("weight each sample by distance ... sampling a
        finite number of points based on distance") and gives no formula for; defined in ``include/svr.h``
        (``SVR_MODE_WEIGHTED_AVERAGE``): sample i weighs ``max(1 - weight_falloff * d_i, 0) ** 2``, the pixel shows
        the weighted mean of the ray's samples at the sample that contributes most.

        "composite": direct volume rendering — front-to-back emission-absorption compositing of every sample's colour
        and opacity from ``transfer_function`` until the ray's opacity reaches ``alpha_cutoff`` (``svr_composite`` in
        ``include/svr.h``).  Hit pixels carry straight alpha; rays that gather no opacity are transparent misses.

        "iso": the iso-surface — the first point along each ray where the density reaches ``iso_value`` (searched
        with ``iso_refine`` sub-samples per step), lit from the local gradient by two-sided Blinn-Phong (``ambient``,
        ``diffuse``, ``specular``, ``shininess_log2``, ``light_direction``) over ``iso_color`` or, with
        ``color_by_label``, the hit label's hue (``svr_iso`` in ``include/svr.h``).  Rays that never reach the level
        are transparent misses."""
        return self._u["render_mode"]

    @render_mode.setter
    def render_mode(self, mode) -> None:
        mode = str(mode).lower()
        if mode not in self.RENDER_MODES:
            raise ValueError(f"render_mode must be one of {self.RENDER_MODES}, not {mode!r}")
        self._store("render_mode", mode)

    # -- interpolation (pygfx's volume materials carry the same property) ---------------------------------------
    INTERPOLATIONS = ("nearest", "linear")

    @property
    def interpolation(self) -> str:
        """"nearest" (the default): every sample is one ring texel, as the reference's ``textureLoad`` reads it.
        "linear": the "composite" and "iso" render modes, and ``render_slice`` / ``render_slab``, blend the eight
        texels around each sample trilinearly inside the LOD the nearest sample picks (``svr_set_interpolation`` in
        ``include/svr.h``); labels are never interpolated.  The march ("lmip", "mip", "weighted_average") samples
        nearest texels only: ``SubVolume.render`` refuses those modes while this is "linear"."""
        return self._u["interpolation"]

    @interpolation.setter
    def interpolation(self, mode) -> None:
        mode = str(mode).lower()
        if mode not in self.INTERPOLATIONS:
            raise ValueError(f"interpolation must be one of {self.INTERPOLATIONS}, not {mode!r}")
        self._store("interpolation", mode)

    @property
    def weight_falloff(self) -> float:
        """"weighted_average" mode: how fast a sample's weight falls with its distance d from the ray's entry
        into the volume (d in the fog's unit: 1 = one volume edge); samples at d >= 1 / weight_falloff weigh
        nothing and are not taken.  0 = plain mean of the whole ray."""
        return float(self._u["weight_falloff"])

    @weight_falloff.setter
    def weight_falloff(self, value) -> None:
        value = float(value)
        if not (0.0 <= value < float("inf")):
            raise ValueError(f"weight_falloff must be finite and >= 0, not {value!r}")
        self._store("weight_falloff", np.float32(value))

    # -- composite mode (svr_composite) --------------------------------------------------------------------
    @property
    def transfer_function(self):
        """The ``TransferFunction`` of the "composite" mode; None (the default) means ``TransferFunction.linear()``."""
        return self._u["transfer_function"]

    @transfer_function.setter
    def transfer_function(self, tf) -> None:
        from ._transfer import TransferFunction

        if tf is not None and not isinstance(tf, TransferFunction):
            raise ValueError(f"transfer_function must be a TransferFunction or None, not {type(tf).__name__}")
        self._store("transfer_function", tf)

    def effective_transfer_function(self):
        """``transfer_function``, or the default one when it is None."""
        from ._transfer import default_transfer_function

        tf = self._u["transfer_function"]
        return default_transfer_function() if tf is None else tf

    @property
    def alpha_cutoff(self) -> float:
        """"composite" mode: a ray stops once its accumulated opacity reaches this value, in (0, 1]."""
        return float(self._u["alpha_cutoff"])

    @alpha_cutoff.setter
    def alpha_cutoff(self, value) -> None:
        if isinstance(value, (str, bytes)) or not isinstance(value, numbers.Real):
            raise ValueError(f"alpha_cutoff must be a number in (0, 1], not {value!r}")
        v = np.float32(float(value))
        if not (0.0 < v <= 1.0):
            raise ValueError(f"alpha_cutoff must be in (0, 1] (as float32), not {value!r}")
        self._store("alpha_cutoff", v)

    @property
    def color_by_label(self) -> bool:
        """"composite" mode: tint each sample's colour by the hue of its label (``colors``)."""
        return bool(self._u["color_by_label"])

    @color_by_label.setter
    def color_by_label(self, value) -> None:
        self._store("color_by_label", bool(value))

    # -- iso mode (svr_iso) ----------------------------------------------------------------------------------
    @staticmethod
    def _real(name, value):
        if isinstance(value, (str, bytes, bool)) or not isinstance(value, numbers.Real):
            raise ValueError(f"{name} must be a number, not {value!r}")
        with np.errstate(over="ignore"):
            return np.float32(float(value))

    @staticmethod
    def _integer(name, value, lo, hi):
        if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not lo <= int(value) <= hi:
            raise ValueError(f"{name} must be an integer in {lo} .. {hi}, not {value!r}")
        return np.int32(int(value))

    @property
    def iso_value(self) -> float:
        """"iso" mode: the level, in the units of the data (compared with the sampled value like ``lmip_threshold``:
        0 .. 255 for uint8 volumes).  +-inf is allowed (nothing / everything reaches it), NaN is not."""
        return float(self._u["iso_value"])

    @iso_value.setter
    def iso_value(self, value) -> None:
        v = self._real("iso_value", value)
        if np.isnan(v):
            raise ValueError("iso_value must not be NaN")
        self._store("iso_value", v)

    @property
    def iso_color(self) -> tuple[float, float, float]:
        """"iso" mode: the surface's base colour, linear-light RGB, each component in [0, 1]."""
        return tuple(float(c) for c in self._u["iso_color"])

    @iso_color.setter
    def iso_color(self, rgb) -> None:
        if isinstance(rgb, (str, bytes)) or not isinstance(rgb, (tuple, list, np.ndarray)) or len(rgb) != 3:
            raise ValueError(f"iso_color must be three numbers in [0, 1], not {rgb!r}")
        vals = np.array([self._real("iso_color", c) for c in rgb], np.float32)
        if not np.all((vals >= 0.0) & (vals <= 1.0)):
            raise ValueError(f"iso_color must be three numbers in [0, 1], not {rgb!r}")
        self._store("iso_color", vals)

    @property
    def iso_refine(self) -> int:
        """"iso" mode: sub-samples per step searched, in order, between the last sample below the level and the first
        one at it (0 or 1: none; at most 16)."""
        return int(self._u["iso_refine"])

    @iso_refine.setter
    def iso_refine(self, value) -> None:
        self._store("iso_refine", self._integer("iso_refine", value, 0, 16))

    def _shading_coefficient(self, name, value):
        v = self._real(name, value)
        if not (0.0 <= v < np.inf):
            raise ValueError(f"{name} must be finite (as float32) and >= 0, not {value!r}")
        self._store(name, v)

    @property
    def ambient(self) -> float:
        """"iso" mode: the share of the base colour shown regardless of the light."""
        return float(self._u["ambient"])

    @ambient.setter
    def ambient(self, value) -> None:
        self._shading_coefficient("ambient", value)

    @property
    def diffuse(self) -> float:
        """"iso" mode: the weight of the Lambert term ``|n . l|``."""
        return float(self._u["diffuse"])

    @diffuse.setter
    def diffuse(self, value) -> None:
        self._shading_coefficient("diffuse", value)

    @property
    def specular(self) -> float:
        """"iso" mode: the weight of the (white) Blinn-Phong highlight ``|n . h| ** (2 ** shininess_log2)``."""
        return float(self._u["specular"])

    @specular.setter
    def specular(self, value) -> None:
        self._shading_coefficient("specular", value)

    @property
    def shininess_log2(self) -> int:
        """"iso" mode: log2 of the specular exponent, 0 .. 10 (the kernel squares that many times)."""
        return int(self._u["shininess_log2"])

    @shininess_log2.setter
    def shininess_log2(self, value) -> None:
        self._store("shininess_log2", self._integer("shininess_log2", value, 0, 10))

    @property
    def light_direction(self):
        """"iso" mode: the world-space direction from the surface towards the light, or None (the default): a
        headlight at the viewer.  Any non-zero finite vector; stored normalised."""
        d = self._u["light_direction"]
        return None if d is None else tuple(float(c) for c in d)

    @light_direction.setter
    def light_direction(self, direction) -> None:
        if direction is None:
            return self._store("light_direction", None)
        if isinstance(direction, (str, bytes)) or not isinstance(direction, (tuple, list, np.ndarray)) or len(direction) != 3:
            raise ValueError(f"light_direction must be None or three numbers, not {direction!r}")
        d = np.array([float(self._real("light_direction", c)) for c in direction], np.float64)
        length = float(np.sqrt((d * d).sum()))
        if not np.all(np.isfinite(d)) or not (0.0 < length < np.inf):
            raise ValueError(f"light_direction must be a finite, non-zero vector, not {direction!r}")
        self._store("light_direction", (d / length).astype(np.float32))

    def lmip_uniforms(self) -> tuple[float, float, int]:
        """(threshold, fall_off, max_samples) as the draw sends them for the current render mode."""
        if self._u["render_mode"] == "mip":
            return float("-inf"), 0.0, 2**31 - 1
        return float(self._u["lmip_threshold"]), float(self._u["lmip_fall_off"]), int(self._u["lmip_max_samples"])

    # -- label hues: list of (h, s, v); stored vec4-padded like the reference's n*4xf4 array (:119-159) ---
    @property
    def _color_count(self):
        return np.uint32(len(self._u["colors"]))

    @property
    def colors(self) -> list[tuple[float, float, float]]:
        """The list of HSV colors used for rendering labels (each padded to four components)."""
        return [tuple(map(float, row)) for row in self._u["colors"]]

    @colors.setter
    def colors(self, hsv_list) -> None:
        if not isinstance(hsv_list, (list, tuple)):
            raise TypeError("Colors must be a list.")
        table = np.ones((len(hsv_list), 4), np.float32)               # fourth component: padding, always 1
        for row, hsv in zip(table, hsv_list):
            if not isinstance(hsv, (list, tuple)) or len(hsv) != 3:
                raise TypeError(f"Each color must be an hsv tuple, not {hsv}")
            row[:3] = hsv
        self._store("colors", table)
