"""ctypes binding of the C ABI in ``include/svr.h`` (libsvr_hip.so).

There is NO fallback: if the HIP library has not been built, or a call fails,
this module raises.  The library is built in-tree by ``__graft_entry__.build()``
(``hipcc --offload-arch=gfx950``).
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVR_LIB") or os.path.join(_HERE, "csrc", "libsvr_hip.so")      # SVR_LIB: A/B builds (tools/ab_build.py)

SVR_MAX_LODS = 8
SVR_PIX_DISCARD, SVR_PIX_MISS, SVR_PIX_HIT = 0, 1, 2

_DTYPES = {
    np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.uint32): 2, np.dtype(np.uint64): 3,
    np.dtype(np.int8): 4, np.dtype(np.int16): 5, np.dtype(np.int32): 6, np.dtype(np.int64): 7,
    np.dtype(np.float32): 8, np.dtype(np.float64): 9,
}


def dtype_code(dt) -> int:
    dt = np.dtype(dt)
    if dt == np.dtype(bool):
        return 0
    try:
        return _DTYPES[dt]
    except KeyError:
        raise TypeError(f"unsupported source dtype {dt} for a ring-buffer upload") from None


class LodDesc(C.Structure):
    _fields_ = [("ring_dims", C.c_int32 * 3), ("density_storage", C.c_int32), ("no_labels", C.c_int32),
                ("blocked_twin", C.c_int32)]


SVR_U8, SVR_U16, SVR_F32 = 0, 1, 8


class LodState(C.Structure):
    _fields_ = [("offset", C.c_int32 * 3), ("shape", C.c_int32 * 3), ("scale", C.c_float * 3)]


class Material(C.Structure):
    _fields_ = [
        ("clim", C.c_float * 2),
        ("gamma", C.c_float),
        ("opacity", C.c_float),
        ("lmip_threshold", C.c_float),
        ("lmip_fall_off", C.c_float),
        ("lmip_max_samples", C.c_int32),
        ("fog_density", C.c_float),
        ("fog_color", C.c_float * 3),
        ("color_count", C.c_uint32),
        ("colors", C.POINTER(C.c_float)),
        ("colorspace_srgb", C.c_int32),
        ("clipping_plane_count", C.c_uint32),
        ("clipping_mode_all", C.c_int32),
        ("clipping_planes", C.POINTER(C.c_float)),
        ("render_mode", C.c_int32),
        ("weight_falloff", C.c_float),
    ]


SVR_MODE_LMIP, SVR_MODE_WEIGHTED_AVERAGE = 0, 1


class Camera(C.Structure):
    _fields_ = [
        ("world", C.c_float * 16),
        ("world_inv", C.c_float * 16),
        ("cam", C.c_float * 16),
        ("cam_inv", C.c_float * 16),
        ("proj", C.c_float * 16),
        ("proj_inv", C.c_float * 16),
        ("volume_dimensions", C.c_float * 3),
    ]


class Frame(C.Structure):
    _fields_ = [
        ("frame_w", C.c_int32), ("frame_h", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32),
        ("out_w", C.c_int32), ("out_h", C.c_int32),
        ("band_h", C.c_int32), ("band_pitch", C.c_int32),
    ]


class Outputs(C.Structure):
    _fields_ = [
        ("rgba", C.c_void_p),
        ("depth", C.c_void_p),
        ("label", C.c_void_p),
        ("flags", C.c_void_p),
        ("steps", C.c_void_p),
        ("pick", C.c_void_p),
        ("pick_id", C.c_uint32),
    ]

    @classmethod
    def of(cls, res, *, steps=False, pick=False, pick_id=0):
        """The struct over the planes of a render result: ``rgba``, and ``depth`` / ``label`` / ``flags`` where the
        result holds them; ``steps`` and ``pick`` only when asked for and present (NULL otherwise)."""
        ob = cls()
        ob.rgba = res.rgba.data_ptr()
        for name in ("depth", "label", "flags"):
            t = getattr(res, name)
            setattr(ob, name, t.data_ptr() if t is not None else None)
        ob.steps = res.steps.data_ptr() if (steps and res.steps is not None) else None
        ob.pick = res.pick.data_ptr() if (pick and res.pick is not None) else None   # the `write_pick` shader variant
        ob.pick_id = pick_id
        return ob


class ComposeParams(C.Structure):
    _fields_ = [("bg_bottom", C.c_float * 4), ("bg_top", C.c_float * 4), ("srgb_encode", C.c_int32)]


class OutlineParams(C.Structure):
    _fields_ = [
        ("radius", C.c_int32),
        ("depth_tolerance", C.c_float),
        ("color_by_label", C.c_int32),
        ("color", C.c_float * 4),
        ("dim_unselected", C.c_float),
        ("only_selected", C.c_int32),
    ]


class SlicePlane(C.Structure):
    _fields_ = [
        ("world_inv", C.c_float * 16),
        ("volume_dimensions", C.c_float * 3),
        ("origin", C.c_float * 3),
        ("u", C.c_float * 3),
        ("v", C.c_float * 3),
    ]


class SliceOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("rgba", "depth", "label", "flags", "value", "lod")]

    @classmethod
    def of(cls, res):
        """The struct over the planes of a slice / slab result; a plane the result leaves out (None) is NULL."""
        ob = cls()
        for name, _ in cls._fields_:
            t = getattr(res, name)
            setattr(ob, name, t.data_ptr() if t is not None else None)
        return ob


class SlabParams(C.Structure):
    _fields_ = [
        ("plane", SlicePlane),
        ("w", C.c_float * 3),
        ("w_len", C.c_float),
        ("samples", C.c_int32),
        ("mode", C.c_int32),
    ]


SLAB_MODES = {"max": 0, "min": 1, "mean": 2}        # SVR_SLAB_*
SLAB_MAX_SAMPLES = 4096


class CompositeParams(C.Structure):
    _fields_ = [("alpha_cutoff", C.c_float), ("color_by_label", C.c_int32)]


TF_MAX_ENTRIES = 4096                               # SVR_TF_MAX_ENTRIES


class IsoParams(C.Structure):
    _fields_ = [
        ("iso_value", C.c_float),
        ("refine", C.c_int32),
        ("iso_color", C.c_float * 3),
        ("color_by_label", C.c_int32),
        ("ambient", C.c_float),
        ("diffuse", C.c_float),
        ("specular", C.c_float),
        ("shininess_log2", C.c_int32),
        ("headlight", C.c_int32),
        ("light_direction", C.c_float * 3),
        ("no_skip", C.c_int32),
        ("normal", C.c_void_p),
        ("skip_counters", C.c_void_p),
    ]


class HistogramParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("bins", C.c_int32),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
    ]


class HistogramOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("counts", "tail", "range")]


HIST_MAX_BINS = 4096                                # SVR_HIST_MAX_BINS


class ObjectsParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
        ("ignore_zero", C.c_int32),
        ("capacity", C.c_uint32),
    ]


class ObjectRecord(C.Structure):
    _fields_ = [
        ("label", C.c_uint32),
        ("used", C.c_uint32),
        ("voxels", C.c_uint64),
        ("sum", C.c_uint64 * 3),
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("finite", C.c_uint64),
        ("value_sum", C.c_uint64),
        ("vmin", C.c_float),
        ("vmax", C.c_float),
        ("reserved", C.c_uint64),
    ]


class ObjectsOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("records", "header")]


OBJECTS_MAX_CAPACITY = 1 << 26                      # SVR_OBJECTS_MAX_CAPACITY
OBJECT_RECORD_BYTES = 96                            # sizeof(svr_object_record)


class ContactsParams(ObjectsParams):                # svr_contacts_params: svr_objects_params' fields
    pass


class ContactRecord(C.Structure):
    _fields_ = [
        ("label_lo", C.c_uint32),
        ("label_hi", C.c_uint32),
        ("faces", C.c_uint64 * 3),
        ("sum2", C.c_uint64 * 3),
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("finite", C.c_uint64),
        ("value_sum", C.c_uint64),
        ("vmin", C.c_float),
        ("vmax", C.c_float),
        ("reserved", C.c_uint64),
    ]


class ContactsOutputs(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("records", "header")]


CONTACTS_MAX_CAPACITY = 1 << 26                     # SVR_CONTACTS_MAX_CAPACITY
CONTACT_RECORD_BYTES = 112                          # sizeof(svr_contact_record)

class MeshParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("mode", C.c_int32),
        ("level", C.c_float),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
    ]


class MeshOutputs(C.Structure):
    _fields_ = [
        ("vertices", C.c_void_p),
        ("triangles", C.c_void_p),
        ("header", C.c_void_p),
        ("vertex_capacity", C.c_uint64),
        ("triangle_capacity", C.c_uint64),
    ]


MESH_LABELS, MESH_LEVEL = 0, 1                      # SVR_MESH_*
MESH_MAX_CELLS = 1 << 28                            # SVR_MESH_MAX_CELLS


class ComponentsParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("mode", C.c_int32),
        ("level", C.c_float),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
        ("ignore_zero", C.c_int32),
        ("join_labels", C.c_int32),
        ("connectivity", C.c_int32),
    ]


class ComponentRecord(C.Structure):
    _fields_ = [
        ("id", C.c_uint32),
        ("label", C.c_uint32),
        ("voxels", C.c_uint64),
        ("sum", C.c_uint64 * 3),
        ("first", C.c_int32 * 3),
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("reserved", C.c_uint32),
    ]


class ComponentsOutputs(C.Structure):
    _fields_ = [
        ("ids", C.c_void_p),
        ("ids_capacity", C.c_uint64),
        ("records", C.c_void_p),
        ("record_capacity", C.c_uint64),
        ("header", C.c_void_p),
    ]


COMPONENTS_LABELS, COMPONENTS_LEVEL = 0, 1          # SVR_COMPONENTS_*
COMPONENTS_MAX_VOXELS = 1 << 30                     # SVR_COMPONENTS_MAX_VOXELS
COMPONENT_RECORD_BYTES = 80                         # sizeof(svr_component_record)


class DistanceParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("mode", C.c_int32),
        ("level", C.c_float),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
        ("ignore_zero", C.c_int32),
        ("invert", C.c_int32),
        ("border", C.c_int32),
    ]


class DistanceOutputs(C.Structure):
    _fields_ = [
        ("d2", C.c_void_p),
        ("d2_capacity", C.c_uint64),
        ("header", C.c_void_p),
    ]


DISTANCE_FAR = 0x7FFFFFFF                           # SVR_DISTANCE_FAR
DISTANCE_MAX_EXTENT = 16384                         # SVR_DISTANCE_MAX_EXTENT
DISTANCE_MAX_VOXELS = 1 << 30                       # SVR_DISTANCE_MAX_VOXELS


class NearestParams(C.Structure):
    _fields_ = [
        ("lod", C.c_int32),
        ("use_box", C.c_int32),
        ("box_off", C.c_int32 * 3),
        ("box_shape", C.c_int32 * 3),
        ("mode", C.c_int32),
        ("level", C.c_float),
        ("selected", C.c_void_p),
        ("selected_count", C.c_uint32),
        ("ignore_zero", C.c_int32),
        ("invert", C.c_int32),
    ]


class NearestOutputs(C.Structure):
    _fields_ = [
        ("d2", C.c_void_p),
        ("index", C.c_void_p),
        ("label", C.c_void_p),
        ("capacity", C.c_uint64),
        ("header", C.c_void_p),
    ]


class SplitParams(C.Structure):
    _fields_ = [
        ("height", C.c_void_p),
        ("n", C.c_int32 * 3),
        ("connectivity", C.c_int32),
        ("merge_squared", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SplitRecord(C.Structure):
    _fields_ = [
        ("id", C.c_uint32),
        ("basins", C.c_uint32),
        ("voxels", C.c_uint64),
        ("sum", C.c_uint64 * 3),
        ("top", C.c_int32 * 3),
        ("lo", C.c_int32 * 3),
        ("hi", C.c_int32 * 3),
        ("peak", C.c_int32),
    ]


class SplitOutputs(C.Structure):
    _fields_ = [
        ("ids", C.c_void_p),
        ("ids_capacity", C.c_uint64),
        ("records", C.c_void_p),
        ("record_capacity", C.c_uint64),
        ("header", C.c_void_p),
    ]


SPLIT_MAX_VOXELS = 1 << 30                          # SVR_SPLIT_MAX_VOXELS
SPLIT_MAX_MERGE = 1 << 29                           # SVR_SPLIT_MAX_MERGE
SPLIT_RECORD_BYTES = 80                             # sizeof(svr_split_record)

INTERPOLATIONS = {"nearest": 0, "linear": 1}      # SVR_INTERP_*
CUT_MODES = {"ANY": 0, "ALL": 1}                  # SVR_CUT_*
MAX_CUT_PLANES = 8                                # SVR_MAX_CUT_PLANES

ISO_MAX_REFINE = 16                                 # SVR_ISO_MAX_REFINE
ISO_MAX_SHININESS_LOG2 = 10                         # SVR_ISO_MAX_SHININESS_LOG2


_I3 = C.c_int32 * 3
_L3 = C.c_int64 * 3

# name -> (restype, argtypes): every symbol include/svr.h declares
SIGNATURES = {
    "svr_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(LodDesc), C.POINTER(C.c_void_p)]),
    "svr_destroy": (C.c_int, [C.c_void_p]),
    "svr_last_error": (C.c_char_p, []),
    "svr_abi_version": (C.c_int, []),
    "svr_set_lod_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LodState)]),
    "svr_get_lod_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LodState)]),
    "svr_set_material": (C.c_int, [C.c_void_p, C.POINTER(Material)]),
    "svr_upload_region": (C.c_int, [C.c_void_p, C.c_int, _I3, _I3,
                                    C.c_void_p, C.c_int, _L3, C.c_void_p, C.c_int, _L3]),
    "svr_upload_region_device": (C.c_int, [C.c_void_p, C.c_int, _I3, _I3,
                                           C.c_void_p, C.c_int, _L3, C.c_void_p, C.c_int, _L3]),
    "svr_publish_uploads": (C.c_int, [C.c_void_p]),
    "svr_mark_uploads": (C.c_int, [C.c_void_p]),
    "svr_uploads_pending": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "svr_upload_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_int]),
    "svr_upload_ticket": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "svr_ticket_pending": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]),
    "svr_read_region": (C.c_int, [C.c_void_p, C.c_int, _I3, _I3, C.c_void_p, C.c_void_p]),
    "svr_clear_lod": (C.c_int, [C.c_void_p, C.c_int]),
    "svr_render": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame),
                             C.POINTER(Outputs), C.c_void_p]),
    "svr_set_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "svr_untile_stripes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_untile_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "svr_comm_unique_id": (C.c_int, [C.c_char * 128]),
    "svr_comm_init": (C.c_int, [C.c_void_p, C.c_char * 128, C.c_int, C.c_int]),
    "svr_comm_destroy": (C.c_int, [C.c_void_p]),
    "svr_gather_tiles": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_size_t), C.c_int, C.c_void_p]),
    "svr_pool2x": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, _I3, C.c_int, C.c_int, C.c_void_p]),
    "svr_compose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                              C.POINTER(ComposeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "svr_outline": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                              C.POINTER(OutlineParams), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "svr_slice": (C.c_int, [C.c_void_p, C.POINTER(SlicePlane), C.POINTER(Frame), C.POINTER(SliceOutputs), C.c_void_p]),
    "svr_slab": (C.c_int, [C.c_void_p, C.POINTER(SlabParams), C.POINTER(Frame), C.POINTER(SliceOutputs), C.c_void_p]),
    "svr_set_transfer_function": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "svr_composite": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.POINTER(CompositeParams),
                                C.POINTER(Outputs), C.c_void_p]),
    "svr_iso": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame), C.POINTER(IsoParams), C.POINTER(Outputs),
                          C.c_void_p]),
    "svr_set_interpolation": (C.c_int, [C.c_void_p, C.c_int]),
    "svr_set_cut_planes": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_int]),
    "svr_histogram": (C.c_int, [C.c_void_p, C.POINTER(HistogramParams), C.POINTER(HistogramOutputs), C.c_void_p]),
    "svr_objects": (C.c_int, [C.c_void_p, C.POINTER(ObjectsParams), C.POINTER(ObjectsOutputs), C.c_void_p]),
    "svr_contacts": (C.c_int, [C.c_void_p, C.POINTER(ContactsParams), C.POINTER(ContactsOutputs), C.c_void_p]),
    "svr_mesh": (C.c_int, [C.c_void_p, C.POINTER(MeshParams), C.POINTER(MeshOutputs), C.c_void_p]),
    "svr_components": (C.c_int, [C.c_void_p, C.POINTER(ComponentsParams), C.POINTER(ComponentsOutputs), C.c_void_p]),
    "svr_distance": (C.c_int, [C.c_void_p, C.POINTER(DistanceParams), C.POINTER(DistanceOutputs), C.c_void_p]),
    "svr_nearest": (C.c_int, [C.c_void_p, C.POINTER(NearestParams), C.POINTER(NearestOutputs), C.c_void_p]),
    "svr_split": (C.c_int, [C.c_void_p, C.POINTER(SplitParams), C.POINTER(SplitOutputs), C.c_void_p]),
    "svr_sync": (C.c_int, [C.c_void_p]),
    "svr_sync_uploads": (C.c_int, [C.c_void_p]),
    "svr_debug_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "svr_debug_timers": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "svr_lod_device_ptrs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "svr_lod_twin_ptr": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "svr_lod_cell_ptrs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _I3,
                                    C.POINTER(C.c_int32)]),
    "svr_time_render": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Frame),
                                  C.POINTER(Outputs), C.c_int, C.POINTER(C.c_float)]),
}

_lib = None


class SvrError(RuntimeError):
    pass


def lib():
    """Load libsvr_hip.so (once).  Raises loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SvrError(
            f"HIP extension not built: {LIB_PATH} is missing. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` in the repo root. "
            "There is no CPU fallback."
        )
    # torch ships the HIP runtime (libamdhip64.so.7) this process must share:
    # import it first so the dynamic loader resolves our NEEDED entry to that copy.
    import torch  # noqa: F401

    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if the symbol is missing: loud
        fn.restype = res
        fn.argtypes = args
    _lib = handle
    return _lib


def check(status: int, what: str = "") -> None:
    if status == 0:
        return
    msg = lib().svr_last_error()
    msg = msg.decode("utf-8", "replace") if msg else ""
    if status == -1:
        raise ValueError(f"{what}: {msg}")
    if status == -3:
        raise MemoryError(f"{what}: {msg}")
    if status == -4:
        raise IndexError(f"{what}: {msg}")
    raise SvrError(f"{what}: status {status}: {msg}")


def i3(v) -> "C.Array":
    return _I3(int(v[0]), int(v[1]), int(v[2]))


def l3(v) -> "C.Array":
    return _L3(int(v[0]), int(v[1]), int(v[2]))


def mat_to_c(m) -> "C.Array":
    """numpy row-major 4x4 -> column-major float[16] (WGSL mat4x4 layout)."""
    a = np.asarray(m, dtype=np.float32).reshape(4, 4)
    return (C.c_float * 16)(*a.T.reshape(-1).tolist())
