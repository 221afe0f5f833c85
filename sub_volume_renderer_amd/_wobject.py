"""``SubVolume`` — the multi-LOD volume object and its draw call.

Mirror of the reference's ``SubVolume(gfx.Volume)``
(``src/sub_volume/_wobject.py:13-226``): same constructor, validation errors,
attributes and ``center_on_position()``.  The reference is drawn by pygfx's
``renderer.render(scene, camera)`` through the plugin in ``_shader.py``; pygfx does
not exist on the target, so the draw is the explicit :meth:`SubVolume.render`,
which hands the camera matrices and the frame region to ``svr_render``
(include/svr.h) — one HIP kernel launch for vs_main + fs_main + raycast.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._geometry import Coordinate, Roi
from ._material import SubVolumeMaterial
from ._transform import _HasWorld
from ._wrapping_buffer import DeviceRings, WrappingBuffer, native_density_storage


@dataclass
class FrameRegion:
    """Which pixels of the full frame one call renders (``svr_frame``)."""

    x0: int = 0
    y0: int = 0
    out_w: int = 0
    out_h: int = 0
    band_h: int = 0       # 0: one contiguous tile
    band_pitch: int = 0

    @staticmethod
    def full(width: int, height: int) -> "FrameRegion":
        return FrameRegion(0, 0, width, height, height, height)

    @staticmethod
    def tile(x0: int, y0: int, w: int, h: int) -> "FrameRegion":
        return FrameRegion(x0, y0, w, h, h, h)

    @staticmethod
    def stripes(width: int, height: int, rank: int, nranks: int, band_h: int = 8) -> "FrameRegion":
        """Rows dealt to ranks round-robin in bands of ``band_h`` rows (padded to equal size)."""
        nbands = -(-height // band_h)
        per_rank = -(-nbands // nranks)
        return FrameRegion(0, rank * band_h, width, per_rank * band_h, band_h, band_h * nranks)


@dataclass
class RenderResult:
    """Device tensors written by one draw (fragment outputs before blending)."""

    rgba: "object"            # torch f32 [h, w, 4]   out.color   (fs_main.wgsl:86,95)
    depth: "object | None"    # torch f32 [h, w]      out.depth   (fs_main.wgsl:72,97)
    label: "object | None"    # torch i32 [h, w]      bit pattern of the u32 label (raycast.wgsl:81)
    flags: "object | None"    # torch u8  [h, w]      0 discard / 1 miss / 2 hit
    steps: "object | None"    # torch i32 [h, w]      executed march iterations (instrumented)
    pick: "object | None" = None   # torch i64 [h, w]   bit pattern of the 64-bit pick word (fs_main.wgsl:89-92)

    def label_numpy(self) -> np.ndarray:
        return self.label.cpu().numpy().view(np.uint32)


@dataclass
class IsoResult(RenderResult):
    """A ``RenderResult`` with the extra planes only the "iso" render mode writes.  Pass one as ``out=`` to
    ``SubVolume.render`` (``SubVolume.iso_outputs`` allocates it): the other modes leave the extra planes alone."""

    normal: "object | None" = None          # torch f32 [h, w, 3]  unit world-space surface normal, 0 on non-hits
    skip_counters: "object | None" = None   # torch i32 [2]        wave-stretches marched / skipped, ADDED per render


@dataclass
class SliceResult(RenderResult):
    """Device tensors written by one cross-section (``svr_slice``): the planes of a render (``steps`` and ``pick`` are
    None, depth is 0) plus the density texel each pixel shows and the LOD it came from."""

    value: "object | None" = None     # torch f32 [h, w]   density texel (0 where nothing was hit)
    lod: "object | None" = None       # torch u8  [h, w]   LOD of that texel (255 where nothing was hit)


_SLICE_PLANES = (("depth", "float32"), ("label", "int32"), ("flags", "uint8"), ("value", "float32"), ("lod", "uint8"))


def _vec3(name, value):
    """Three numbers that are finite as float32, the precision the kernel works in (a str is not a vector)."""
    if isinstance(value, (str, bytes)):
        raise ValueError(f"{name} must be three finite numbers")
    try:
        vals = np.array([float(c) for c in value], np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three finite numbers") from None
    if vals.shape != (3,) or not np.all(np.isfinite(vals)):
        raise ValueError(f"{name} must be three finite numbers")
    with np.errstate(over="ignore"):
        vals = vals.astype(np.float32)
    if not np.all(np.isfinite(vals)):
        raise ValueError(f"{name} must be three numbers that are finite in float32")
    return [float(c) for c in vals]


_HIST_WIDE = 2.0 ** 100     # float32 rings, range=None: the K = 1 pass that only takes min and max runs over (-2^100, 2^100)


@dataclass
class HistogramResult:
    """What one ``svr_histogram`` call wrote (include/svr.h).  ``counts`` stays on the device; the scalars are read
    from the device (after a synchronisation) the first time one of them is asked for."""

    counts: "object"          # torch i64 [bins]     voxels per bin (bit pattern of the u64 counts)
    tail: "object"            # torch i64 [4]        under, over, NaN, considered
    range: "object"           # torch f32 [2]        min and max of the considered non-NaN values
    edges: np.ndarray         # float64 [bins + 1]   bin j is [edges[j], edges[j + 1]), the last one closed
    lod: int
    selected: "object | None" = None    # torch i32 [n]  the sorted id list the kernel searched (kept alive with the result)
    _host: "tuple | None" = None

    def _scalars(self):
        if self._host is None:
            import torch

            torch.cuda.synchronize(self.counts.device)
            t, r = self.tail.cpu().numpy(), self.range.cpu().numpy()
            self._host = (int(t[0]), int(t[1]), int(t[2]), int(t[3]), float(r[0]), float(r[1]))
        return self._host

    under = property(lambda self: self._scalars()[0], doc="considered voxels below the range")
    over = property(lambda self: self._scalars()[1], doc="considered voxels above the range")
    nan = property(lambda self: self._scalars()[2], doc="considered voxels that are NaN")
    considered = property(lambda self: self._scalars()[3], doc="voxels considered: sum(counts) + under + over + nan")
    min = property(lambda self: self._scalars()[4], doc="smallest considered non-NaN value (+inf: none)")
    max = property(lambda self: self._scalars()[5], doc="largest considered non-NaN value (-inf: none)")


def histogram_edges(lo: float, hi: float, bins: int) -> np.ndarray:
    """The K + 1 bin edges of a histogram over the float32 range [lo, hi], in float64."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + (hi - lo) * (np.arange(bins + 1, dtype=np.float64) / float(bins))


def clim_from_counts(counts, edges, percentiles=(0.5, 99.5)):
    """Contrast limits from a histogram's counts alone, in float64: with N = sum(counts) and c_j their cumulative sum,
    the left edge of the first bin with c_j > N * p_lo / 100 and the right edge of the first bin with
    c_j >= N * p_hi / 100; one bin width apart when the two coincide.  ``ValueError`` when N == 0."""
    counts = np.asarray(counts, np.float64).reshape(-1)
    edges = np.asarray(edges, np.float64).reshape(-1)
    if len(edges) != len(counts) + 1:
        raise ValueError("edges must hold one more entry than counts")
    try:
        p_lo, p_hi = (float(p) for p in percentiles)
    except (TypeError, ValueError):
        raise ValueError("percentiles must be two numbers") from None
    if not 0.0 <= p_lo <= p_hi <= 100.0:
        raise ValueError("percentiles must satisfy 0 <= low <= high <= 100")
    total = counts.sum()
    if not total > 0:
        raise ValueError("auto_clim: the histogram is empty (nothing resident in the box, or every voxel outside the range)")
    cum = np.cumsum(counts)
    k = len(counts)
    j_lo = min(int(np.argmax(cum > total * p_lo / 100.0)) if (cum > total * p_lo / 100.0).any() else k - 1, k - 1)
    j_hi = min(int(np.argmax(cum >= total * p_hi / 100.0)) if (cum >= total * p_hi / 100.0).any() else k - 1, k - 1)
    lower, upper = float(edges[j_lo]), float(edges[j_hi + 1])
    if upper <= lower:                 # only with low == high, when a cumulative count meets the target exactly
        upper = lower + float(edges[j_lo + 1] - edges[j_lo])
    return lower, upper


def label_ids(labels) -> np.ndarray:
    """An iterable of label ids -> the sorted, unique uint32 array ``svr_histogram`` searches."""
    if isinstance(labels, (str, bytes)):
        raise ValueError("labels must be an iterable of integer ids")
    try:
        vals = [v for v in labels]
    except TypeError:
        raise ValueError("labels must be an iterable of integer ids") from None
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError("labels must hold integers")
    if not vals:
        raise ValueError("labels must hold at least one id (None counts every voxel)")
    if min(int(v) for v in vals) < 0 or max(int(v) for v in vals) > 0xFFFFFFFF:
        raise ValueError("label ids must lie in [0, 2^32)")
    return np.unique(np.array([int(v) for v in vals], np.uint64)).astype(np.uint32)


def lod_box(begin, end, scale_factor):
    """A voxel box ``[begin, end)`` of the finest scale (numpy order, the convention of ``crop_planes``) in the voxels
    of a LOD with ``scale_factor``: ``(floor(begin * scale), ceil(end * scale))`` per axis, as ints (numpy order)."""
    begin = np.asarray(begin, np.float64).reshape(-1)
    end = np.asarray(end, np.float64).reshape(-1)
    if begin.shape != (3,) or end.shape != (3,) or not (np.all(np.isfinite(begin)) and np.all(np.isfinite(end))):
        raise ValueError("begin and end must be three finite numbers each")
    if not np.all(end > begin):
        raise ValueError("end must exceed begin on every axis")
    scale = np.asarray(scale_factor, np.float64)
    b, e = np.floor(begin * scale), np.ceil(end * scale)
    if np.any(np.abs(b) >= 2.0 ** 31) or np.any(np.abs(e) >= 2.0 ** 31) or np.any(e - b >= 2.0 ** 31):
        raise ValueError("the box does not fit 32-bit voxel coordinates")
    return tuple(int(v) for v in b), tuple(int(v) for v in e)


_OBJECTS_FIRST_CAPACITY = 4096      # records of the first pass of ``SubVolume.objects(capacity=None)``; 8 times more per rerun


def objects_capacity(capacity, id_count=None):
    """``(records of the first pass, automatic)`` of ``SubVolume.objects``: an explicit integer capacity in
    1 .. SVR_OBJECTS_MAX_CAPACITY runs once; None starts at ``_OBJECTS_FIRST_CAPACITY``, or at the number of ids when
    ``labels`` are given, which can never overflow."""
    if capacity is None:
        return (_OBJECTS_FIRST_CAPACITY if id_count is None else int(id_count)), True
    if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= N.OBJECTS_MAX_CAPACITY:
        raise ValueError(f"capacity must be None or an integer in 1 .. {N.OBJECTS_MAX_CAPACITY}")
    return int(capacity), False


def finest_box(begin, end, scale_factor):
    """The inverse of :func:`lod_box`: the voxel box ``[begin, end)`` of a LOD with ``scale_factor`` (numpy order) in
    voxels of the finest scale, ``(floor(begin / scale), ceil(end / scale))`` per axis, as ints."""
    scale = np.asarray(scale_factor, np.float64).reshape(-1)
    b = np.floor(np.asarray(begin, np.float64).reshape(-1) / scale)
    e = np.ceil(np.asarray(end, np.float64).reshape(-1) / scale)
    return tuple(int(v) for v in b), tuple(int(v) for v in e)


def lod_center_to_data(center, scale_factor):
    """A point in a LOD's voxel coordinates (integer c: the centre of voxel c; any order, ``scale_factor`` in the same
    one) as a data coordinate of the finest scale.  LOD voxel c covers the finest index interval [c / scale,
    (c + 1) / scale) and finest voxel i is centred on data coordinate i (it covers [i - 0.5, i + 0.5), the convention of
    :meth:`SubVolume.crop_planes`), so the centre maps to ``(c + 0.5) / scale - 0.5``."""
    c = np.asarray(center, np.float64)
    return (c + 0.5) / np.asarray(scale_factor, np.float64) - 0.5


def lod_center_to_world(volume, center, scale_factor):
    """A point in a LOD's voxel coordinates (numpy order, as :func:`lod_center_to_data` reads it) as a world-space
    position (x, y, z) under ``volume``'s world transform, for :meth:`SubVolume.center_on_position`."""
    data = lod_center_to_data(center, scale_factor)[::-1]     # shader order
    world = np.asarray(volume.world.matrix, np.float64) @ np.array([*data, 1.0])
    return tuple(float(v) for v in world[:3])


@dataclass
class ObjectTable:
    """The occupied records of one ``svr_objects`` call (include/svr.h), compacted and sorted by id on the device.
    Coordinates are LOD voxels in numpy order (z, y, x)."""

    ids: "object"             # torch i64 [n]        the labels, ascending
    voxels: "object"          # torch i64 [n]
    begin: "object"           # torch i64 [n, 3]     smallest voxel coordinate
    end: "object"             # torch i64 [n, 3]     largest voxel coordinate + 1
    centroid: "object"        # torch f64 [n, 3]     window offset + sum / voxels
    finite: "object"          # torch i64 [n]        voxels whose value is finite
    mean: "object"            # torch f64 [n]        of the finite values; NaN where there are none
    min: "object"             # torch f32 [n]        +inf where finite == 0
    max: "object"             # torch f32 [n]        -inf where finite == 0
    considered: int           # voxels that took part
    background: int           # label-0 voxels left out by background=False
    lod: int
    scale_factor: tuple = (1.0, 1.0, 1.0)       # of the LOD, numpy order
    volume: "object | None" = None              # the SubVolume, for its world transform
    _host: "dict | None" = None

    def __len__(self):
        return int(self.ids.numel())

    def _rows(self):
        if self._host is None:
            self._host = {k: getattr(self, k).cpu().numpy() for k in ("ids", "begin", "end", "centroid")}
        return self._host

    def index(self, label) -> int:
        """The row of ``label``; ``KeyError`` when the table does not hold it."""
        ids = self._rows()["ids"]
        i = int(np.searchsorted(ids, int(label)))
        if i >= len(ids) or int(ids[i]) != int(label):
            raise KeyError(label)
        return i

    def box(self, label):
        """``(begin, end)`` of the object's bounding box in voxels of the finest scale (numpy order, ints), ready for
        :meth:`SubVolume.crop_planes` and ``histogram(box=)``: :func:`finest_box` of its LOD box."""
        i = self.index(label)
        rows = self._rows()
        return finest_box(rows["begin"][i], rows["end"][i], self.scale_factor)

    def position(self, label):
        """The world-space position (x, y, z) of the object's centroid, for :meth:`SubVolume.center_on_position`: the
        centroid in LOD voxels mapped to the finest data coordinate by :func:`lod_center_to_data`
        (``(c + 0.5) / scale - 0.5``), then through the volume's world transform."""
        i = self.index(label)
        data = lod_center_to_data(self._rows()["centroid"][i], self.scale_factor)[::-1]       # shader order
        world = np.asarray(self.volume.world.matrix, np.float64) @ np.array([*data, 1.0])
        return tuple(float(v) for v in world[:3])


_SLICE_CACHE_SIZES = 4      # output sets kept per volume: e.g. the three axis views of a viewer, each of its own size


def _stop_upload_worker(jobs_queue, thread):
    """Let the upload thread finish what it holds and end (called by ``SubVolume.close`` or when a volume is collected)."""
    import threading

    jobs_queue.put(None)
    if thread.is_alive() and thread is not threading.current_thread():
        thread.join(timeout=30.0)


class SubVolume(_HasWorld):
    material: SubVolumeMaterial

    def __init__(
        self,
        material: SubVolumeMaterial,
        data_segmentation_pairs,
        buffer_shape_in_chunks,
        chunk_shape_in_pixels=None,
        *,
        device: int | None = None,
        ring_storage: str = "native",
        blocked_twin="auto",
    ):
        super().__init__()
        pairs = list(data_segmentation_pairs)
        levels = len(pairs)
        finest = pairs[0][0]

        # One value for every scale (a tuple) or one value per scale (any other sequence, whose length
        # must then equal the number of scales) — the two spellings the reference accepts (_wobject.py:34-63).
        def per_scale(value, name):
            if isinstance(value, tuple):
                return [value] * levels
            if len(value) != levels:
                raise ValueError(f"{name} list length ({len(value)}) must match number of scales ({levels})")
            return value

        buffer_shapes = per_scale(buffer_shape_in_chunks, "buffer_shape_in_chunks")
        if chunk_shape_in_pixels is None:
            # chunked array types (zarr, tensorstore) know their own chunking (_wobject.py:46-53)
            native = getattr(finest, "chunks", None)
            if native is None:
                raise ValueError("if chunk_shape_in_pixels is not provided, base data must have a 'chunks' attribute")
            chunk_shape_in_pixels = tuple(native)
        chunk_shapes = per_scale(chunk_shape_in_pixels, "chunk_shape_in_pixels")
        for level, ((density, _), chunk) in enumerate(zip(pairs, chunk_shapes)):
            if len(chunk) != density.ndim:
                raise ValueError(f"chunk_shape_in_pixels[{level}] length must match data dimensions")
        data_segmentation_pairs, num_scales, base_data = pairs, levels, finest
        # segmentations are optional here (the reference wishes for it, FUTURE.md:178-193): either every scale has
        # one or none has; without them no label ring exists and every hit is coloured with colors[0]
        unlabelled = [seg is None for _, seg in pairs]
        if any(unlabelled) and not all(unlabelled):
            raise ValueError("either every scale has a segmentation array or none has")
        if num_scales > N.SVR_MAX_LODS:
            raise ValueError(f"at most {N.SVR_MAX_LODS} scales are supported")

        self.material = material
        # all LODs share one device context (one svr_ctx); created lazily on first device use
        self._rings = DeviceRings(
            [tuple(Coordinate(b) * Coordinate(c)) for b, c in zip(buffer_shapes, chunk_shapes)],
            device=device,
            # "native": byte rings when every density source is uint8 (identical results, 4x less
            # memory traffic); "float32": always the reference's r32float layout
            density_storage=native_density_storage([d for d, _ in data_segmentation_pairs], ring_storage),
            labels=not all(unlabelled),
            # "auto": the finest scale's density ring is kept in two layouts — rows, and 128-byte micro-blocks that are
            # compact in 3-D; each wave of the march gathers from the one that suits its view (include/svr.h)
            blocked_twin=blocked_twin,
        )
        self.wrapping_buffers: list[WrappingBuffer] = []
        for i, (scale_data, scale_segmentations) in enumerate(data_segmentation_pairs):
            # same-sized voxels: lower resolutions sample at scaled-down coordinates (_wobject.py:79-81)
            scale_factor = tuple(float(scale_data.shape[j]) / float(base_data.shape[j]) for j in range(3))
            self.wrapping_buffers.append(
                WrappingBuffer(
                    backing_data=scale_data,
                    segmentations=scale_segmentations,
                    shape_in_chunks=buffer_shapes[i],
                    chunk_shape_in_pixels=chunk_shapes[i],
                    scale_factor=scale_factor,
                    _rings=self._rings,
                    _lod=i,
                )
            )
        self._volume_dimensions = np.zeros(3, np.float32)
        self.volume_dimensions = base_data.shape
        self._material_version_pushed = -1
        self.iso_no_skip = False          # "iso" mode: march every stretch (A/B of the empty-space skipping; same frame)
        self._tf_pushed = None            # (TransferFunction, volume_dimensions bytes) of the table on the device
        # pygfx gives every world object a process-wide id (the shader packs its low 20 bits into the pick word)
        SubVolume._next_id = getattr(SubVolume, "_next_id", 0) + 1
        self.id = SubVolume._next_id
        self._out_cache = {}
        self._cam_cache = None
        self._frame_cache = {}
        self._ob_cache = {}
        self._slice_cache = {}
        self._slab_cache = {}         # separate: a slab never overwrites the tensors of the last slice
        self._worker = None
        self._worker_error = None
        self._inflight = []
        self._submitted = 0
        self._completed = 0

    # -- _wobject.py:103-133 ---------------------------------------------------
    @property
    def volume_dimensions(self):
        """The dimensions of the volume in pixels, numpy axis order."""
        return tuple(self._volume_dimensions[::-1])

    @volume_dimensions.setter
    def volume_dimensions(self, value):
        # stored reversed = shader order, like the reference's uniform (_wobject.py:121-123)
        self._volume_dimensions = np.array(tuple(value)[::-1], dtype=np.float32)

    @property
    def textures(self):
        """All scale level textures."""
        return [b.texture for b in self.wrapping_buffers]

    @property
    def segmentations_textures(self):
        """All scale level segmentation textures."""
        return [b.segmentations_texture for b in self.wrapping_buffers]

    # -- _wobject.py:135-208 ---------------------------------------------------
    def center_on_position(self, position, sizes=None, *, asynchronous: bool = False):
        """Center every LOD's ring window on a world position (x, y, z).

        ``asynchronous=True`` (not in the reference, whose uploads block the render thread —
        FUTURE.md:3-7): the call only plans the loads and publishes the shrunk ROIs; the chunk copies
        run on a worker thread / the upload stream beside later renders, and :meth:`render` publishes
        the full new ROIs once they have landed (:meth:`poll_uploads`).

        ``sizes``: window size per scale in that scale's voxels (numpy order).  By
        default one chunk less than the ring per axis, so that growing the window
        to the chunk grid can never exceed the ring (_wobject.py:151-177).
        """
        if sizes is None:
            sizes = [
                (b.shape_in_chunks - Coordinate(1, 1, 1)) * b.chunk_shape_in_pixels
                for b in self.wrapping_buffers
            ]
        if len(sizes) != len(self.wrapping_buffers):
            raise ValueError(
                f"sizes list length ({len(sizes)}) must match number of scales ({len(self.wrapping_buffers)})"
            )
        # world -> data space; the matrix works in shader order, so reverse to numpy order
        p = (self.world.inverse_matrix @ np.array([*position, 1.0]))[:3][::-1]
        if not asynchronous and self._submitted != self._completed:
            self.poll_uploads(wait=True)                  # never interleave a blocking load with the worker's
        jobs = []
        for size, buffer in zip(sizes, self.wrapping_buffers):
            offset = tuple(int(c * f - s // 2) for c, s, f in zip(p, size, buffer.scale_factor))
            roi = Roi(offset, size)
            if buffer.can_load_logical_roi(roi):
                if asynchronous:
                    buffer._async_focus = tuple(c * f for c, f in zip(p, buffer.scale_factor))
                    pieces = buffer.begin_async_load(roi)
                    if pieces:
                        jobs.append((buffer, pieces))
                else:
                    buffer.load_logical_roi(roi)
        if jobs:
            self._submit_uploads(jobs)

    def close(self):
        """Stop the upload thread (after the loads it already holds) and free the rings and every other device
        allocation of this volume now, instead of when the object is collected."""
        stop = getattr(self, "_worker_stop", None)
        if stop is not None:
            stop()
        self._worker = None
        self._inflight.clear()
        self._completed = self._submitted
        self._out_cache, self._ob_cache, self._slice_cache, self._slab_cache = {}, {}, {}, {}
        self._rings.close()

    # -- asynchronous streaming ------------------------------------------------------
    @staticmethod
    def _prioritise(jobs):
        """Upload order "low res near > low res far > high res near > high res far" (FUTURE.md:86-95): the
        coarsest level first — it covers the most space, and it is what the sampler falls back to while a
        finer level's window is shrunk — and inside a level the pieces nearest to the camera first."""
        ordered = []
        for buffer, pieces in sorted(jobs, key=lambda job: -job[0]._lod):
            focus = getattr(buffer, "_async_focus", None)
            if focus is not None:
                chunk = buffer.chunk_shape_in_pixels

                def distance2(piece, focus=focus, chunk=chunk):
                    roi = piece[1]                                           # logical ROI in chunks
                    return sum(((b + 0.5 * n) * c - f) ** 2 for b, n, c, f in zip(roi.begin, roi.shape, chunk, focus))

                pieces = sorted(pieces, key=distance2)
            ordered.append((buffer, pieces))
        return ordered

    def _submit_uploads(self, jobs):
        import queue
        import threading

        import weakref

        handle = self._rings.handle                       # create the context on this thread
        for b in self.wrapping_buffers:
            b._async_owner = weakref.ref(self)
        if self._worker is None:
            # the thread holds the queue, the result list and the context handle — not the volume: a volume that is
            # dropped is collected, and its finalizer stops the thread BEFORE the device context goes away
            jobs_queue = self._jobs = queue.Queue()
            inflight = self._inflight

            def run():
                lib = N.lib()
                while True:
                    item = jobs_queue.get()
                    if item is None:
                        return
                    buffer, pieces = item
                    ticket, error = C.c_uint64(0), None
                    try:
                        for buffer_roi, logical_roi in pieces:
                            buffer.load_into_buffer(buffer_roi, logical_roi)
                        N.check(lib.svr_upload_ticket(handle, C.byref(ticket)), "svr_upload_ticket")
                    except BaseException as exc:          # surfaced by poll_uploads on the render thread
                        error = exc
                    inflight.append((buffer, ticket.value, error))
                    del item, buffer, pieces              # an idle thread keeps no level (and through it no volume) alive

            self._worker = threading.Thread(target=run, name="svr-upload", daemon=True)
            self._worker.start()
            self._worker_stop = weakref.finalize(self, _stop_upload_worker, jobs_queue, self._worker)
        # one job per level, coarse levels first: each gets its own ticket and is published as soon as
        # ITS chunks have landed
        for job in self._prioritise(jobs):
            self._submitted += 1
            self._jobs.put(job)

    def poll_uploads(self, wait: bool = False) -> bool:
        """Publish the full ROI of every asynchronous load whose chunks have landed in HBM.
        Returns True when nothing is in flight any more.  An exception raised by a backing array on the
        worker thread is re-raised here, once; that level keeps its shrunk window and re-plans next time."""
        import time

        lib = N.lib()
        while True:
            errors, replay = [], []
            while self._inflight:
                buffer, ticket, error = self._inflight[0]
                if error is None:
                    pending = C.c_int(0)
                    N.check(lib.svr_ticket_pending(self._rings.handle, ticket, C.byref(pending)), "svr_ticket_pending")
                    if pending.value:
                        break
                self._inflight.pop(0)
                self._completed += 1
                if error is None:
                    wanted = buffer.finish_async_load()
                else:
                    errors.append(error)
                    wanted = buffer.abort_async_load()
                if wanted is not None:
                    replay.append((buffer, wanted))
            jobs = []
            for buffer, roi in replay:                     # requests that arrived meanwhile: the latest one wins
                if buffer.can_load_logical_roi(roi):
                    pieces = buffer.begin_async_load(roi)
                    if pieces:
                        jobs.append((buffer, pieces))
            if jobs:
                self._submit_uploads(jobs)
            if errors:
                raise errors[0]
            if self._submitted == self._completed or not wait:
                return self._submitted == self._completed
            time.sleep(0.0002)

    # -- the draw --------------------------------------------------------------
    def _push_material(self):
        m = self.material
        if self._material_version_pushed == m._version:
            return
        u = m._u
        cm = N.Material()
        cm.clim[:] = [float(u["clim"][0]), float(u["clim"][1])]
        cm.gamma = float(u["gamma"])
        cm.opacity = float(u["opacity"])
        cm.lmip_threshold, cm.lmip_fall_off, cm.lmip_max_samples = m.lmip_uniforms()
        cm.fog_density = float(u["fog_density"])
        cm.fog_color[:] = [float(v) for v in u["fog_color"]]
        colors = np.ascontiguousarray(u["colors"], np.float32)
        cm.color_count = int(colors.shape[0])
        cm.colors = colors.ctypes.data_as(C.POINTER(C.c_float))
        # _shader.py:68: colorspace of the first texture; 'srgb' selects srgb2physical
        cm.colorspace_srgb = 1 if self.textures[0].colorspace == "srgb" else 0
        planes = np.ascontiguousarray(u["clipping_planes"], np.float32)
        cm.clipping_plane_count = int(planes.shape[0])
        cm.clipping_mode_all = 1 if u["clipping_mode"] == "ALL" else 0
        cm.clipping_planes = planes.ctypes.data_as(C.POINTER(C.c_float))
        # "composite" sends LMIP here: svr_composite does not read the mode (its table goes through _push_transfer_function)
        cm.render_mode = N.SVR_MODE_WEIGHTED_AVERAGE if u["render_mode"] == "weighted_average" else N.SVR_MODE_LMIP
        cm.weight_falloff = float(u["weight_falloff"])
        N.check(N.lib().svr_set_material(self._rings.handle, C.byref(cm)), "svr_set_material")
        self._material_version_pushed = m._version

    def _push_transfer_function(self):
        """Send the composite mode's table (alpha corrected for this volume's sample spacing) when the transfer
        function or ``volume_dimensions`` changed since the last one sent."""
        tf = self.material.effective_transfer_function()
        key = (tf, self._volume_dimensions.tobytes())
        pushed = self._tf_pushed
        if pushed is not None and pushed[0] is key[0] and pushed[1] == key[1]:
            return
        table = np.ascontiguousarray(tf.device_table(self._volume_dimensions), np.float32)
        N.check(N.lib().svr_set_transfer_function(self._rings.handle, table.ctypes.data, table.shape[0]),
                "svr_set_transfer_function")
        self._tf_pushed = key

    def _push_interpolation(self, interpolation=None):
        """Set the context's sampling for the next slice / slab / composite / iso call: ``interpolation``, or the
        material's when it is None."""
        mode = self.material.interpolation if interpolation is None else str(interpolation).lower()
        if mode not in N.INTERPOLATIONS:
            raise ValueError(f"interpolation must be one of {tuple(N.INTERPOLATIONS)} or None, not {interpolation!r}")
        N.check(N.lib().svr_set_interpolation(self._rings.handle, N.INTERPOLATIONS[mode]), "svr_set_interpolation")

    def _push_cut_planes(self):
        """Set the context's cut planes for the next composite / iso call from the material (an empty list too, so
        that a material change clears the context)."""
        planes = np.ascontiguousarray(self.material._u["cut_planes"], np.float32).reshape(-1, 4)
        mode = N.CUT_MODES[self.material.cut_mode]
        ptr = planes.ctypes.data_as(C.POINTER(C.c_float)) if len(planes) else None
        N.check(N.lib().svr_set_cut_planes(self._rings.handle, ptr, len(planes), mode), "svr_set_cut_planes")

    def crop_planes(self, begin, end):
        """The six world-space planes (a, b, c, d) of the voxel box ``[begin, end)`` (numpy order, like the array's
        indices) under the volume's current world transform, computed in float64: with ``material.cut_mode = "ANY"``
        and ``material.cut_planes = volume.crop_planes(begin, end)`` the "composite" and "iso" renders are cropped to
        the box.  Voxel i of an axis covers [i - 0.5, i + 0.5) in data space, so the box is [begin - 0.5, end - 0.5)."""
        begin = np.asarray(begin, np.float64).reshape(-1)
        end = np.asarray(end, np.float64).reshape(-1)
        if begin.shape != (3,) or end.shape != (3,) or not (np.all(np.isfinite(begin)) and np.all(np.isfinite(end))):
            raise ValueError("begin and end must be three finite numbers each")
        if not np.all(end > begin):
            raise ValueError("end must exceed begin on every axis")
        inv = np.asarray(self.world.inverse_matrix, np.float64)        # world -> data (x, y, z)
        planes = []
        for axis in range(3):                                           # numpy axis; the data-space axis is 2 - axis
            row = inv[2 - axis]
            lo, hi = begin[axis] - 0.5, end[axis] - 0.5
            # kept: lo <= dot(row[:3], w) + row[3] < hi
            planes.append((row[0], row[1], row[2], lo - row[3]))
            planes.append((-row[0], -row[1], -row[2], row[3] - hi))
        return [tuple(float(v) for v in p) for p in planes]

    def _camera_key(self, camera):
        # the projection enters as the bytes of its matrix, whatever kind of camera made it: every parameter of
        # any projection (fov, width, height, zoom, aspect, depth range) changes the key exactly when it changes
        # the matrix
        w, cw = self.world, camera.world
        return (id(camera), w._position.tobytes(), w._rot.tobytes(), w._scale.tobytes(),
                cw._position.tobytes(), cw._rot.tobytes(), cw._scale.tobytes(),
                np.asarray(camera.projection_matrix, np.float64).tobytes(), self._volume_dimensions.tobytes())

    def camera_block(self, camera) -> "N.Camera":
        """The uniforms vs_main/fs_main read, as ``svr_camera`` (cached while nothing moved)."""
        key = self._camera_key(camera) if hasattr(camera, "near_far") else None
        if key is not None and self._cam_cache is not None and self._cam_cache[0] == key:
            return self._cam_cache[1]
        cb = self._camera_block_uncached(camera)
        self._cam_cache = (key, cb)
        return cb

    def _camera_block_uncached(self, camera) -> "N.Camera":
        cb = N.Camera()
        cb.world = N.mat_to_c(self.world.matrix)
        cb.world_inv = N.mat_to_c(self.world.inverse_matrix)
        cb.cam = N.mat_to_c(camera.view_matrix)
        cb.cam_inv = N.mat_to_c(camera.camera_matrix)
        cb.proj = N.mat_to_c(camera.projection_matrix)
        cb.proj_inv = N.mat_to_c(camera.projection_matrix_inverse)
        cb.volume_dimensions[:] = [float(v) for v in self._volume_dimensions]
        return cb

    def frame_block(self, width: int, height: int, region: FrameRegion | None) -> "N.Frame":
        r = region or FrameRegion.full(width, height)
        key = (width, height, r.x0, r.y0, r.out_w, r.out_h, r.band_h, r.band_pitch)
        fb = self._frame_cache.get(key)
        if fb is not None:
            return fb
        fb = self._frame_cache[key] = N.Frame()
        fb.frame_w, fb.frame_h = int(width), int(height)
        fb.x0, fb.y0, fb.out_w, fb.out_h = int(r.x0), int(r.y0), int(r.out_w), int(r.out_h)
        fb.band_h = int(r.band_h or r.out_h)
        fb.band_pitch = int(r.band_pitch or r.out_h)
        return fb

    def _outputs(self, h, w, want_steps, want_pick=False):
        import torch

        key = (h, w, bool(want_steps), bool(want_pick))
        res = self._out_cache.get(key)
        if res is None:
            dev = torch.device("cuda", self._rings.device if self._rings.device is not None else torch.cuda.current_device())
            res = RenderResult(
                rgba=torch.empty((h, w, 4), dtype=torch.float32, device=dev),
                depth=torch.empty((h, w), dtype=torch.float32, device=dev),
                label=torch.empty((h, w), dtype=torch.int32, device=dev),
                flags=torch.empty((h, w), dtype=torch.uint8, device=dev),
                steps=torch.empty((h, w), dtype=torch.int32, device=dev) if want_steps else None,
                pick=torch.empty((h, w), dtype=torch.int64, device=dev) if want_pick else None,
            )
            self._out_cache = {key: res}
        return res

    def iso_outputs(self, width: int, height: int, *, count_steps: bool = False, pick: bool = False,
                    normal: bool = True, skip_counters: bool = False) -> "IsoResult":
        """Fresh output tensors for an "iso" render of ``height`` x ``width`` output pixels, with the normal plane
        and / or the two skip counters (zeroed; every render adds to them), for ``render(..., out=...)``."""
        import torch

        dev = torch.device("cuda", self._rings.device if self._rings.device is not None else torch.cuda.current_device())
        h, w = int(height), int(width)
        return IsoResult(
            rgba=torch.empty((h, w, 4), dtype=torch.float32, device=dev),
            depth=torch.empty((h, w), dtype=torch.float32, device=dev),
            label=torch.empty((h, w), dtype=torch.int32, device=dev),
            flags=torch.empty((h, w), dtype=torch.uint8, device=dev),
            steps=torch.empty((h, w), dtype=torch.int32, device=dev) if count_steps else None,
            pick=torch.empty((h, w), dtype=torch.int64, device=dev) if pick else None,
            normal=torch.empty((h, w, 3), dtype=torch.float32, device=dev) if normal else None,
            skip_counters=torch.zeros(2, dtype=torch.int32, device=dev) if skip_counters else None,
        )

    def _iso_params(self, res) -> "N.IsoParams":
        """The ``svr_iso_params`` of the material's "iso" settings; ``res``: the outputs (an ``IsoResult``'s extra
        planes are written)."""
        m = self.material
        ip = N.IsoParams()
        ip.iso_value = m.iso_value
        ip.refine = m.iso_refine
        ip.iso_color[:] = m.iso_color
        ip.color_by_label = 1 if m.color_by_label else 0
        ip.ambient, ip.diffuse, ip.specular = m.ambient, m.diffuse, m.specular
        ip.shininess_log2 = m.shininess_log2
        light = m.light_direction
        ip.headlight = 1 if light is None else 0
        ip.light_direction[:] = (0.0, 0.0, 1.0) if light is None else light
        ip.no_skip = 1 if self.iso_no_skip else 0
        normal = getattr(res, "normal", None)
        counters = getattr(res, "skip_counters", None)
        ip.normal = normal.data_ptr() if normal is not None else None
        ip.skip_counters = counters.data_ptr() if counters is not None else None
        return ip

    def prepare(self):
        """Push pending uniforms (material, per-LOD ROI/scale) to the device."""
        handle = self._rings.handle  # creates the context on first use
        if self._submitted != self._completed:
            self.poll_uploads()
        self._push_material()
        for b in self.wrapping_buffers:
            b._push_state()
        return handle

    def render(self, camera, width: int, height: int, *, region: FrameRegion | None = None,
               count_steps: bool = False, out: RenderResult | None = None, stream=None,
               pick: bool = False) -> RenderResult:
        """Draw this volume as seen by ``camera`` into device tensors.

        Replaces ``renderer.render(scene, camera)`` for the (SubVolume,
        SubVolumeMaterial) pair (scripts/multi_scale.py:76-80).  Asynchronous:
        the kernel is enqueued on the current torch stream.
        """
        import torch

        if self.material.interpolation == "linear" and self.material.render_mode not in ("composite", "iso"):
            raise ValueError(
                f"render_mode {self.material.render_mode!r} is the march, which samples nearest texels (the reference's "
                "behaviour); interpolation='linear' applies to the render modes 'composite' and 'iso' and to "
                "render_slice / render_slab (pass interpolation='linear' to those calls to keep this material nearest)")
        if len(self.material._u["cut_planes"]) and self.material.render_mode not in ("composite", "iso"):
            raise ValueError(
                f"render_mode {self.material.render_mode!r} is the march, which knows no cut planes (it keeps the "
                "reference's behaviour); cut_planes are honoured by the render modes 'composite' and 'iso' "
                "(svr_composite and svr_iso), not by 'lmip', 'mip', 'weighted_average', render_slice or render_slab")
        handle = self.prepare()
        cb = self.camera_block(camera)
        fb = self.frame_block(width, height, region)
        res = out or self._outputs(fb.out_h, fb.out_w, count_steps, pick)
        okey = (id(res), bool(count_steps), bool(pick))
        cached = self._ob_cache.get(okey)
        if cached is not None and cached[0] is res:
            ob = cached[1]
        else:
            ob = N.Outputs.of(res, steps=count_steps, pick=pick, pick_id=self.id & 0xFFFFFFFF)
            if len(self._ob_cache) > 8:
                self._ob_cache.clear()
            self._ob_cache[okey] = (res, ob)
        if stream is None:
            stream = torch.cuda.current_stream(self._rings.device).cuda_stream
        if self.material.render_mode == "composite":
            # direct volume rendering (svr_composite): same camera block, frame and outputs; its steps plane is
            # written by the production kernel
            self._push_transfer_function()
            self._push_interpolation()
            self._push_cut_planes()
            cp = N.CompositeParams(self.material.alpha_cutoff, 1 if self.material.color_by_label else 0)
            N.check(N.lib().svr_composite(handle, C.byref(cb), C.byref(fb), C.byref(cp), C.byref(ob), C.c_void_p(stream)),
                    "svr_composite")
            return res
        if self.material.render_mode == "iso":
            # lit iso-surface (svr_iso): same camera block, frame and outputs; its steps plane is written by the
            # production kernel
            ip = self._iso_params(res)
            self._push_interpolation()
            self._push_cut_planes()
            N.check(N.lib().svr_iso(handle, C.byref(cb), C.byref(fb), C.byref(ip), C.byref(ob), C.c_void_p(stream)), "svr_iso")
            return res
        N.check(
            N.lib().svr_render(handle, C.byref(cb), C.byref(fb), C.byref(ob), C.c_void_p(stream)),
            "svr_render",
        )
        return res

    # -- cross-sections ---------------------------------------------------------
    @staticmethod
    def axis_slice_plane(axis, center, pixel_size: float = 1.0):
        """``(origin, u, v)`` of the axis-aligned slice through the world point ``center`` whose normal is the world
        ``axis`` ("x", "y", "z" or 0, 1, 2), ``pixel_size`` world units per pixel: z-normal u = +x, v = +y; y-normal
        u = +x, v = +z; x-normal u = +y, v = +z."""
        key = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        if isinstance(key, bool) or key not in (0, 1, 2):
            raise ValueError("axis must be 'x', 'y', 'z', 0, 1 or 2")
        origin = tuple(_vec3("center", center))
        p = float(pixel_size)
        with np.errstate(over="ignore"):
            finite32 = bool(np.isfinite(np.float32(p)))
        if not (finite32 and p > 0.0):
            raise ValueError("pixel_size must be finite and > 0")
        ua, va = {2: (0, 1), 1: (0, 2), 0: (1, 2)}[key]
        u, v = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        u[ua], v[va] = p, p
        return origin, tuple(u), tuple(v)

    def _slice_outputs(self, h, w):
        return self._plane_outputs(self._slice_cache, h, w)

    def _slab_outputs(self, h, w):
        return self._plane_outputs(self._slab_cache, h, w)

    def _plane_outputs(self, cache, h, w):
        import torch

        res = cache.pop((h, w), None)
        if res is None:
            dev = torch.device("cuda", self._rings.device if self._rings.device is not None else torch.cuda.current_device())
            res = SliceResult(
                rgba=torch.empty((h, w, 4), dtype=torch.float32, device=dev),
                depth=torch.empty((h, w), dtype=torch.float32, device=dev),
                label=torch.empty((h, w), dtype=torch.int32, device=dev),
                flags=torch.empty((h, w), dtype=torch.uint8, device=dev),
                steps=None,
                value=torch.empty((h, w), dtype=torch.float32, device=dev),
                lod=torch.empty((h, w), dtype=torch.uint8, device=dev),
            )
            while len(cache) >= _SLICE_CACHE_SIZES:
                del cache[next(iter(cache))]      # least recently used
        cache[(h, w)] = res
        return res

    def _check_slice_out(self, out, h, w):
        import torch

        if not isinstance(out, SliceResult):
            raise ValueError("out must be a SliceResult")
        if out.rgba is None:
            raise ValueError("out.rgba is required")
        planes = [(n, getattr(out, n), dt, s) for n, dt, s in
                  [("rgba", "float32", (h, w, 4))] + [(n, dt, (h, w)) for n, dt in _SLICE_PLANES] if getattr(out, n) is not None]
        for name, t, dt, shape in planes:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous tensor of shape {list(shape)}")
            if t.dtype != getattr(torch, dt):
                raise ValueError(f"out.{name} must have dtype {dt}")
        for name, t, _, _ in planes:
            if t.device.type != "cuda" or (self._rings.device is not None and t.device.index != self._rings.device):
                raise ValueError(f"out.{name} must be on the volume's GPU device")

    def render_slice(self, origin, u, v, width: int, height: int, *, region: FrameRegion | None = None,
                     out: SliceResult | None = None, stream=None, interpolation: str | None = None) -> SliceResult:
        """Sample the multi-LOD rings on a world-space plane into device tensors (definition: ``svr_slice`` in
        include/svr.h).  ``origin`` is the world position of the image centre, ``u`` / ``v`` the world steps from one
        column / row to the next (rows go down the image); world coordinates are those of the camera positions passed
        to :meth:`render` (the volume's ``world`` transform applies).  Every pixel shows the voxel a ray sample at its
        centre would read: the finest resident LOD's texel, or with ``interpolation`` "linear" (None: the material's
        setting) the trilinear blend of the eight texels around it.  Asynchronous on the current torch stream.  Unless ``out`` is
        given, the output tensors of a size are reused by the next call of that size (the last few sizes are kept), so
        a result is overwritten by the next slice of its size."""
        origin, u, v, width, height = self._plane_args(origin, u, v, width, height)
        fb = self._plane_frame(region, out, width, height)
        handle = self.prepare()
        self._push_interpolation(interpolation)
        res = out or self._slice_outputs(fb.out_h, fb.out_w)
        pl = self._plane_struct(origin, u, v)
        N.check(N.lib().svr_slice(handle, C.byref(pl), C.byref(fb), C.byref(self._plane_ob(res)),
                                  C.c_void_p(self._plane_stream(stream))), "svr_slice")
        return res

    def render_slab(self, origin, u, v, w, samples: int, width: int, height: int, *, mode: str = "max",
                    region: FrameRegion | None = None, out: SliceResult | None = None, stream=None,
                    interpolation: str | None = None) -> SliceResult:
        """Thick-slab projection (definition: ``svr_slab`` in include/svr.h): ``samples`` slices of
        :meth:`render_slice`'s plane stacked along the world step ``w`` and centred on it (sample k lies
        ``k - (samples - 1) / 2`` steps off the plane), reduced per pixel over the samples that hit a resident voxel:
        ``mode`` "max" / "min" (value, label, LOD and depth of the winning sample, ties to the first) or "mean" (the mean
        of the values; label, LOD and depth of the sample "max" picks).  ``depth`` is the winner's signed world offset
        from the centre plane, so ``outline(..., depth_tolerance=)`` applies.  Returns the planes of a slice; its
        output tensors are kept per size apart from the slices', so a slab never overwrites the last slice.
        ``interpolation`` as in :meth:`render_slice`: every sample's value is the linear sample."""
        origin, u, v, width, height = self._plane_args(origin, u, v, width, height)
        w = _vec3("w", w)
        f32 = np.float32
        with np.errstate(all="ignore"):
            normal = np.cross(np.array(u, f32), np.array(v, f32))
            triple = f32(np.dot(normal, np.array(w, f32)))
        if not triple != 0:
            raise ValueError("w must not be coplanar with u and v")
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= N.SLAB_MAX_SAMPLES:
            raise ValueError(f"samples must be an integer in 1 .. {N.SLAB_MAX_SAMPLES}")
        if not isinstance(mode, str) or mode not in N.SLAB_MODES:
            raise ValueError("mode must be 'max', 'min' or 'mean'")
        # the data-space step, in float32 in svr_slab's order, and |w| as the kernel receives it
        m = np.asarray(self.world.inverse_matrix, np.float64).astype(f32)
        w32 = np.array(w, f32)
        with np.errstate(all="ignore"):
            dw = [(m[k, 0] * w32[0] + m[k, 1] * w32[1]) + m[k, 2] * w32[2] for k in range(3)]
            w_len = f32(np.linalg.norm(w32.astype(np.float64)))
        if not (np.all(np.isfinite(dw)) and np.isfinite(w_len)):
            raise ValueError("w must have a length and a data-space step that are finite in float32")
        fb = self._plane_frame(region, out, width, height)
        handle = self.prepare()
        self._push_interpolation(interpolation)
        res = out or self._slab_outputs(fb.out_h, fb.out_w)
        sp = N.SlabParams()
        sp.plane = self._plane_struct(origin, u, v)
        sp.w[:] = w
        sp.w_len, sp.samples, sp.mode = float(w_len), int(samples), N.SLAB_MODES[mode]
        N.check(N.lib().svr_slab(handle, C.byref(sp), C.byref(fb), C.byref(self._plane_ob(res)),
                                 C.c_void_p(self._plane_stream(stream))), "svr_slab")
        return res

    @staticmethod
    def axis_slab_plane(axis, center, pixel_size: float = 1.0, step: float = 1.0):
        """``(origin, u, v, w)`` of the axis-aligned slab centred on the world point ``center``: ``origin``, ``u`` and
        ``v`` as :meth:`axis_slice_plane`, ``w`` along +``axis`` with length ``step`` (world units between samples)."""
        origin, u, v = SubVolume.axis_slice_plane(axis, center, pixel_size)
        s = float(step)
        with np.errstate(over="ignore"):
            finite32 = bool(np.isfinite(np.float32(s)))
        if not (finite32 and s > 0.0):
            raise ValueError("step must be finite and > 0")
        w = [0.0, 0.0, 0.0]
        w[{"x": 0, "y": 1, "z": 2}.get(axis, axis)] = s
        return origin, u, v, tuple(w)

    # -- the argument handling slices and slabs share ---------------------------------------
    @staticmethod
    def _plane_args(origin, u, v, width, height):
        origin, u, v = _vec3("origin", origin), _vec3("u", u), _vec3("v", v)
        for name, n in (("width", width), ("height", height)):
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
                raise ValueError(f"{name} must be an integer >= 1")
        with np.errstate(all="ignore"):
            normal = np.cross(np.array(u, np.float32), np.array(v, np.float32))      # float32, as the kernel steps
        if not np.any(normal != 0):
            raise ValueError("u and v must be nonzero and not parallel")
        return origin, u, v, int(width), int(height)

    def _plane_frame(self, region, out, width, height):
        if region is not None:
            stripes = 0 < region.band_h < region.out_h
            if (region.x0 < 0 or region.y0 < 0 or region.out_w < 1 or region.out_h < 1
                    or region.x0 + region.out_w > width
                    or (region.y0 >= height if stripes else region.y0 + region.out_h > height)):
                raise ValueError(f"region {region} does not fit the {width} x {height} frame")
        fb = self.frame_block(width, height, region)
        if out is not None:
            self._check_slice_out(out, fb.out_h, fb.out_w)
        return fb

    def _plane_struct(self, origin, u, v):
        pl = N.SlicePlane()
        pl.world_inv = N.mat_to_c(self.world.inverse_matrix)
        pl.volume_dimensions[:] = [float(c) for c in self._volume_dimensions]
        pl.origin[:], pl.u[:], pl.v[:] = origin, u, v
        return pl

    @staticmethod
    def _plane_ob(res):
        return N.SliceOutputs.of(res)

    def _plane_stream(self, stream):
        import torch

        return torch.cuda.current_stream(self._rings.device).cuda_stream if stream is None else stream

    # -- passes over one LOD's resident window: what histogram() and objects() share ------
    def _check_lod(self, lod):
        if isinstance(lod, bool) or not isinstance(lod, (int, np.integer)) or not 0 <= lod < len(self.wrapping_buffers):
            raise ValueError(f"lod must be an integer in 0 .. {len(self.wrapping_buffers) - 1}")
        return int(lod)

    def _box_params(self, params, lod, box):
        """``box=(begin, end)`` of the finest scale into ``use_box`` / ``box_off`` / ``box_shape`` of a params struct."""
        if box is None:
            return
        try:
            begin, end = box
        except (TypeError, ValueError):
            raise ValueError("box must be (begin, end)") from None
        b, e = lod_box(begin, end, self.wrapping_buffers[lod].scale_factor)
        params.use_box = 1
        params.box_off[:] = b[::-1]                                   # shader order
        params.box_shape[:] = [ev - bv for bv, ev in zip(b[::-1], e[::-1])]

    @staticmethod
    def _upload_ids(params, ids, dev, side):
        """The sorted id list as a device tensor behind ``selected`` / ``selected_count`` of a params struct -> the
        tensor (None without ids).  ``side``: the caller's stream as a torch stream, or None for torch's current one."""
        import torch

        if ids is None:
            return None
        sel = torch.from_numpy(ids.view(np.int32)).to(dev)
        if side is not None:
            # the id list was copied on torch's stream and is read on the caller's: the copy must have landed, and
            # the caching allocator must not hand the memory out again before that stream has passed the kernel
            torch.cuda.current_stream(dev).synchronize()
            sel.record_stream(side)
        params.selected, params.selected_count = sel.data_ptr(), int(sel.numel())
        return sel

    # -- what values are resident? ------------------------------------------------
    def histogram(self, lod: int = 0, bins: int = 256, range=None, box=None, labels=None, stream=None) -> HistogramResult:
        """Intensity histogram of what LOD ``lod`` holds in HBM (definition: ``svr_histogram`` in include/svr.h): one
        pass over the ring on the device, nothing is read back.  ``range=(lo, hi)``: the binned interval, closed at
        ``hi``; None: (0, 256) on uint8 rings, (0, 65536) on uint16 rings, and on float32 rings the minimum and maximum
        of the considered values, found by a first pass (``ValueError`` when nothing is resident, the values are all
        equal, or one of them is infinite).  ``box=(begin, end)``: only the voxels of that box of the finest scale
        (numpy order, the convention of :meth:`crop_planes`), mapped to the LOD by floor(begin * scale) and
        ceil(end * scale); None: the LOD's whole resident window.  ``labels``: count only voxels whose label is one of
        these ids (a volume without segmentation reads label 0 everywhere).  Asynchronous on the current torch stream
        (or ``stream``); the volume's pending uniforms are pushed and asynchronous uploads polled first, as
        :meth:`render_slice` does."""
        import torch

        lod = self._check_lod(lod)
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= N.HIST_MAX_BINS:
            raise ValueError(f"bins must be an integer in 1 .. {N.HIST_MAX_BINS}")
        bins = int(bins)
        storage = self._rings.density_storage
        if range is not None:
            try:
                lo, hi = (float(v) for v in range)
            except (TypeError, ValueError):
                raise ValueError("range must be two numbers (lo, hi)") from None
            with np.errstate(over="ignore"):
                lo32, hi32 = np.float32(lo), np.float32(hi)
            if not (np.isfinite(lo32) and np.isfinite(hi32) and lo32 < hi32):
                raise ValueError("range must be finite in float32 with lo < hi")
        hp = N.HistogramParams()
        hp.lod = lod
        self._box_params(hp, lod, box)
        ids = label_ids(labels) if labels is not None else None
        handle = self.prepare()
        dev = torch.device("cuda", self._rings.device)
        side = torch.cuda.ExternalStream(int(stream), device=dev) if stream is not None else None
        sel = self._upload_ids(hp, ids, dev, side)
        stream = self._plane_stream(stream)

        def run(lo, hi, k):
            counts = torch.empty(k, dtype=torch.int64, device=dev)
            tail = torch.empty(4, dtype=torch.int64, device=dev)
            rng = torch.empty(2, dtype=torch.float32, device=dev)
            hp.lo, hp.hi, hp.bins = lo, hi, k
            ho = N.HistogramOutputs(counts.data_ptr(), tail.data_ptr(), rng.data_ptr())
            N.check(N.lib().svr_histogram(handle, C.byref(hp), C.byref(ho), C.c_void_p(stream)), "svr_histogram")
            if side is not None:                                      # outputs dropped early must outlive the kernel too
                for t in (counts, tail, rng):
                    t.record_stream(side)
            return HistogramResult(counts, tail, rng, histogram_edges(lo, hi, k), lod, selected=sel)

        if range is None:
            if storage == "uint8":
                lo, hi = 0.0, 256.0
            elif storage == "uint16":
                lo, hi = 0.0, 65536.0
            else:
                first = run(-_HIST_WIDE, _HIST_WIDE, 1)
                lo, hi = first.min, first.max                         # synchronises
                if not lo <= hi:
                    raise ValueError("histogram: nothing is resident in the box (pass range=)")
                if lo == hi:
                    raise ValueError(f"histogram: every considered value equals {lo} (pass range=)")
        return run(float(np.float32(lo)), float(np.float32(hi)), bins)

    def auto_clim(self, percentiles=(0.5, 99.5), lod=None, bins=None, range=None, box=None, labels=None):
        """Contrast limits ``(low, high)`` that clip ``percentiles`` of the resident values, from :meth:`histogram`'s
        counts (:func:`clim_from_counts`; values outside ``range`` do not count).  ``lod=None``: the coarsest LOD that
        has a window, which covers the most space for the fewest bytes.  ``bins=None``: 256 on uint8 rings, else 4096.
        Only returns the pair: assign it to ``material.clim``."""
        try:
            p_lo, p_hi = (float(p) for p in percentiles)
        except (TypeError, ValueError):
            raise ValueError("percentiles must be two numbers") from None
        if not 0.0 <= p_lo <= p_hi <= 100.0:
            raise ValueError("percentiles must satisfy 0 <= low <= high <= 100")
        if lod is None:
            if self._submitted != self._completed:
                self.poll_uploads()
            resident = [i for i, b in enumerate(self.wrapping_buffers) if b._current_logical_roi_in_pixels is not None]
            if not resident:
                raise ValueError("auto_clim: no LOD has a resident window")
            lod = resident[-1]
        if bins is None:
            bins = 256 if self._rings.density_storage == "uint8" else N.HIST_MAX_BINS
        res = self.histogram(lod=lod, bins=bins, range=range, box=box, labels=labels)
        return clim_from_counts(res.counts.cpu().numpy(), res.edges, (p_lo, p_hi))

    # -- which objects are resident? ----------------------------------------------
    def objects(self, lod: int = 0, box=None, labels=None, background: bool = False, capacity=None, stream=None) -> ObjectTable:
        """Per-object measurements of what LOD ``lod`` holds in HBM (definition: ``svr_objects`` in include/svr.h): one
        pass over the label and density rings on the device -> one row per resident label with its voxel count,
        bounding box, centroid, and the mean, minimum and maximum of its values.  ``box`` and ``labels`` mean what they
        mean in :meth:`histogram`.  ``background=False`` leaves the voxels of label 0 out (they are counted in
        ``ObjectTable.background``).  ``capacity``: the records of the device table; None starts at
        ``_OBJECTS_FIRST_CAPACITY`` (or at the number of ``labels``) and reruns the pass with 8 times more while labels
        found no record, up to ``SVR_OBJECTS_MAX_CAPACITY`` (then ``ValueError``); an explicit integer runs once and
        raises ``ValueError`` when the table was too small.  The call SYNCHRONISES: the header of every pass is read
        from the device (on ``stream`` when one is given) before the table is compacted and sorted with torch ops."""
        import torch

        lod = self._check_lod(lod)
        ids = label_ids(labels) if labels is not None else None
        cap, automatic = objects_capacity(capacity, None if ids is None else len(ids))
        op = N.ObjectsParams()
        op.lod = lod
        op.ignore_zero = 0 if background else 1
        scale = tuple(float(v) for v in self.wrapping_buffers[lod].scale_factor)
        self._box_params(op, lod, box)
        handle = self.prepare()
        dev = torch.device("cuda", self._rings.device)
        side = torch.cuda.ExternalStream(int(stream), device=dev) if stream is not None else None
        sel = self._upload_ids(op, ids, dev, side)                    # held until the passes below have run
        stream = self._plane_stream(stream)
        while True:
            records = torch.empty((cap, N.OBJECT_RECORD_BYTES // 8), dtype=torch.int64, device=dev)
            header = torch.empty(8, dtype=torch.int64, device=dev)
            if side is not None:
                torch.cuda.current_stream(dev).synchronize()          # the allocator's memory may still be in use there
            op.capacity = cap
            oo = N.ObjectsOutputs(records.data_ptr(), header.data_ptr())
            N.check(N.lib().svr_objects(handle, C.byref(op), C.byref(oo), C.c_void_p(stream)), "svr_objects")
            if side is not None:
                for t in (records, header):
                    t.record_stream(side)
                side.synchronize()
            head = [int(v) for v in header.cpu().numpy()]             # synchronises
            if head[2] == 0:
                break
            if not automatic:
                raise ValueError(f"objects: capacity {cap} is too small: {head[2]} of {head[1]} voxels belong to labels "
                                 f"that found no record (pass a larger capacity, or None)")
            if cap >= N.OBJECTS_MAX_CAPACITY:
                raise ValueError(f"objects: more than {N.OBJECTS_MAX_CAPACITY} distinct labels are resident")
            cap = min(cap * 8, N.OBJECTS_MAX_CAPACITY)
        # compact and sort on the device; record fields by their 4- and 8-byte columns (svr_object_record)
        w32 = records.view(torch.int32)
        rows = torch.nonzero(w32[:, 1] == 1).reshape(-1)
        label = w32[rows, 0].to(torch.int64) & 0xFFFFFFFF
        label, order = torch.sort(label)
        rows = rows[order]
        r64, r32 = records[rows], w32[rows]
        voxels, finite = r64[:, 1], r64[:, 8]
        offset = torch.tensor([head[4], head[5], head[6]], dtype=torch.int64, device=dev)      # read as int64: signed already
        centroid = (offset.to(torch.float64) + r64[:, 2:5].to(torch.float64) / voxels.to(torch.float64).unsqueeze(1)).flip(1)
        if self._rings.density_storage == "float32":
            total = r64[:, 9].contiguous().view(torch.float64)
        else:
            total = r64[:, 9].to(torch.float64)
        mean = torch.where(finite > 0, total / finite.to(torch.float64), torch.full_like(total, float("nan")))
        vmm = r32[:, 20:22].contiguous().view(torch.float32)
        return ObjectTable(ids=label, voxels=voxels.contiguous(), begin=r32[:, 10:13].flip(1).to(torch.int64),
                           end=r32[:, 13:16].flip(1).to(torch.int64) + 1, centroid=centroid, finite=finite.contiguous(), mean=mean,
                           min=vmm[:, 0].contiguous(), max=vmm[:, 1].contiguous(), considered=head[1], background=head[3], lod=lod,
                           scale_factor=scale, volume=self)

    # -- what does an object touch? ---------------------------------------------------
    def contacts(self, lod: int = 0, box=None, labels=None, background: bool = False, capacity=None, stream=None):
        """The contacts between the objects that LOD ``lod`` holds in HBM (definition: ``svr_contacts`` in
        include/svr.h): one pass over the label ring on the device -> :class:`~.contacts.ContactTable`, one row per
        unordered pair of labels that share a voxel face, with the contact area per face normal, its bounding box and
        mean face centre, and the mean, minimum and maximum of the values on both sides of the faces.  ``box`` and
        ``labels`` mean what they mean in :meth:`objects`; ``labels`` reads "the contacts of these objects with
        anything".  Nothing beyond box and window is known, so a voxel on their border has no face outward.
        ``background=False`` leaves the faces with label 0 out (they are counted in ``ContactTable.background``);
        ``background=True`` keeps them: an object's contact with 0 is its free surface.  ``capacity``: the records of
        the device table; None starts at :meth:`objects`' first capacity and reruns the pass with 8 times more while
        pairs found no record, up to ``SVR_CONTACTS_MAX_CAPACITY`` (then ``ValueError``); an explicit integer runs once
        and raises ``ValueError`` when the table was too small.  The call SYNCHRONISES, as :meth:`objects` does."""
        from .contacts import contacts

        return contacts(self, lod=lod, box=box, labels=labels, background=background, capacity=capacity, stream=stream)

    # -- that object, or that level, as a surface ------------------------------------
    def mesh(self, labels=None, level=None, lod: int = 0, box=None, stream=None):
        """The surface of a picked object or of a level set of what LOD ``lod`` holds in HBM, extracted on the device
        (definition: ``svr_mesh`` in include/svr.h; naive surface nets) -> :class:`~.mesh.SurfaceMesh`.  Exactly one of
        ``labels`` (the voxels whose label is one of these ids are inside; a volume without segmentation reads label 0
        everywhere) and ``level`` (the voxels whose value is >= ``level`` are inside; the ring's own units, like the iso
        value) must be given, else ``ValueError``.  ``box`` means what it means in :meth:`histogram`; everything
        outside box and window is outside, so the surface is closed, with flat caps where the box cuts the object.  The
        call SYNCHRONISES twice: it counts first, allocates exactly, then emits.  An empty mesh is a valid result."""
        from .mesh import mesh

        return mesh(self, labels=labels, level=level, lod=lod, box=box, stream=stream)

    # -- how many pieces, how big, which one is under the cursor? -----------------------
    def components(self, level=None, labels=None, background: bool = False, join: bool = False, connectivity: int = 6, lod: int = 0,
                   box=None, stream=None):
        """The connected components of what LOD ``lod`` holds in HBM, labelled on the device (definition:
        ``svr_components`` in include/svr.h) -> :class:`~.components.ComponentLabels`: a dense volume of component
        numbers and one row per component (voxel count, first voxel, bounding box, centroid, label), numbered like
        ``scipy.ndimage.label``.  With ``level`` the voxels whose value is >= ``level`` are inside (the ring's own units,
        like the iso value): the blobs of a level set.  Without it the segmentation decides: ``labels`` (None: every
        label) are inside, ``background=False`` leaves the voxels of label 0 out (they are counted in
        ``ComponentLabels.background``), and neighbours connect only where their labels are equal, so a label that lies
        in five pieces gives five components, unless ``join=True`` joins the inside voxels whatever their labels.
        ``level`` together with ``labels``, and a ``connectivity`` other than 6 (faces) or 26 (faces, edges, corners),
        raise ``ValueError``.  ``box`` means what it means in :meth:`histogram`; nothing connects across the border of box
        and window.  The call SYNCHRONISES twice: it counts first, allocates exactly, then emits."""
        from .components import components

        return components(self, level=level, labels=labels, background=background, join=join, connectivity=connectivity, lod=lod,
                          box=box, stream=stream)

    # -- how thick, where is the deepest point, what is left after eroding by r? -----------
    def distance(self, level=None, labels=None, background: bool = False, invert: bool = False, border: bool = True, signed: bool = False,
                 lod: int = 0, box=None, stream=None):
        """The exact Euclidean distance transform of what LOD ``lod`` holds in HBM, computed on the device (definition:
        ``svr_distance`` in include/svr.h) -> :class:`~.distance.DistanceField`: the squared distance, in LOD voxels, of
        every inside voxel to the nearest voxel that is not inside, as int32, with the largest one and where it lies.
        ``level``, ``labels`` and ``background`` decide what is inside exactly as in :meth:`components`.
        ``border=True`` counts everything beyond box and window as not inside, so an object that the box cuts is thin
        there; ``border=False`` knows nothing beyond the box (the convention of scipy), and an object that fills the box
        is ``FAR`` from everything.  ``invert=True`` gives the distance of every voxel that is NOT inside to the nearest
        inside one (``border`` is not read).  ``signed=True`` makes both calls (``invert`` is not read) and returns
        ``squared`` = d2(inside) - d2(outside): positive inside, negative outside; a side without any source stays
        ``+FAR`` or ``-FAR``.  ``level`` together with ``labels`` raises ``ValueError``.  ``box`` means what it means in
        :meth:`histogram`.  The call SYNCHRONISES twice: it counts first, allocates exactly, then emits."""
        from .distance import distance

        return distance(self, level=level, labels=labels, background=background, invert=invert, border=border, signed=signed, lod=lod,
                        box=box, stream=stream)

    # -- which source is nearest, what are the objects grown by r voxels? --------------------
    def nearest(self, level=None, labels=None, background: bool = False, invert: bool = False, with_labels: bool = True, lod: int = 0,
                box=None, stream=None):
        """The nearest source of every voxel of what LOD ``lod`` holds in HBM, computed on the device (definition:
        ``svr_nearest`` in include/svr.h) -> :class:`~.nearest.NearestField`: what :meth:`distance` gives with
        ``border=False`` and, for every voxel, which voxel that distance is measured to (``index``) and the label there
        (``label``; ``with_labels=False`` leaves it out).  ``level``, ``labels``, ``background`` and ``invert`` mean what
        they mean in :meth:`distance`; nothing beyond box and window is a source.  Among the sources at the smallest
        distance the first in (z, y, x) order is taken, so two calls agree.  With ``invert=True`` over the segmentation
        every background voxel gets the label of the nearest object: see :meth:`expand_labels`.  ``box`` means what it
        means in :meth:`histogram`.  The call SYNCHRONISES twice: it counts first, allocates exactly, then emits."""
        from .nearest import nearest

        return nearest(self, level=level, labels=labels, background=background, invert=invert, with_labels=with_labels, lod=lod, box=box,
                       stream=stream)

    def expand_labels(self, r, labels=None, lod: int = 0, box=None):
        """The objects of the segmentation (``labels``; None: every label but 0) grown by ``r`` voxels without merging
        them, as a dense u32 volume on the device: every voxel outside them that lies at most ``r`` voxels from one takes
        the label of the nearest (``skimage.segmentation.expand_labels``), the others are 0.  The same as
        ``nearest(labels=labels, invert=True).expanded(r)``."""
        from .nearest import expand_labels

        return expand_labels(self, r, labels=labels, lod=lod, box=box)

    # -- which of the objects that touch in one blob is this voxel part of? -----------------
    def split(self, level=None, labels=None, background: bool = False, merge: float = 1.0, connectivity: int = 26, border: bool = True,
              lod: int = 0, box=None, distance=None, stream=None):
        """Touching objects split apart on the device (definition: ``svr_split`` in include/svr.h): the watershed of the
        squared distances of :meth:`distance` -> :class:`~.split.SplitLabels`, a dense volume of region numbers and one
        row per region (voxel count, deepest voxel and the distance there, bounding box, centroid).  Every inside voxel
        climbs, neighbour by neighbour under ``connectivity`` (6 or 26), to the deepest point it can reach; two such
        basins stay one region where the lower of their two depths is less than ``merge`` voxels above the depth of the
        pass between them, so ``merge=0`` keeps every summit apart (but for plateaus) and a large ``merge`` gives the
        connected components back.  ``merge * merge`` is at most 2^29.  ``level``, ``labels``, ``background``,
        ``border``, ``lod`` and ``box`` go to :meth:`distance`, which makes the field; or pass the
        :class:`~.distance.DistanceField` you already hold as ``distance=`` (then ``level`` and ``labels`` raise
        ``ValueError``): a ``signed=True`` field splits its inside, an ``invert=True`` field the space between the
        objects.  The call SYNCHRONISES twice: it counts first, allocates exactly, then emits."""
        from .split import split

        return split(self, level=level, labels=labels, background=background, merge=merge, connectivity=connectivity, border=border,
                     lod=lod, box=box, distance=distance, stream=stream)

    def synchronize(self):
        N.check(N.lib().svr_sync(self._rings.handle), "svr_sync")
