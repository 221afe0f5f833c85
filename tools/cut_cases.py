"""The cut planes the timing tools use (`--cut`), derived from a camera's position and focus:
  none   no planes;
  half   one plane through the focus, facing the camera: the half of the scene towards the camera is removed (ANY);
  wedge  the three axis planes through the focus, each facing the camera's side of it: that octant is removed (ALL)."""
import ctypes as C

import numpy as np

CUTS = ("none", "half", "wedge")


def cut_case(name, eye, focus):
    """(planes, mode) for SubVolumeMaterial.cut_planes / cut_mode."""
    eye, focus = np.asarray(eye, np.float64), np.asarray(focus, np.float64)
    if name == "none":
        return [], "ANY"
    if name == "half":
        n = (focus - eye) / np.linalg.norm(focus - eye)
        return [tuple(float(v) for v in n) + (float(n @ focus),)], "ANY"
    if name != "wedge":
        raise ValueError(f"unknown cut {name!r}")
    planes = []
    for a in range(3):
        s = 1.0 if eye[a] >= focus[a] else -1.0            # cut where s * (w_a - focus_a) > 0
        n = [0.0, 0.0, 0.0]
        n[a] = -s
        planes.append(tuple(n) + (float(-s * focus[a]),))
    return planes, "ALL"


def names_of(arg):
    return CUTS if arg == "all-cases" else (arg,)


def push(lib, handle, planes, mode, modes):
    """svr_set_cut_planes through the C ABI (the timed calls bypass the Python layer); ``modes``: _native.CUT_MODES."""
    flat = (C.c_float * max(4 * len(planes), 1))(*[v for p in planes for v in p])
    return lib.svr_set_cut_planes(handle, flat if planes else None, len(planes), modes[mode])
