"""What ``mesh()``, ``components()`` and ``distance()`` share, the three passes over a box of one LOD's resident window
that count first, allocate exactly and then emit: the check of ``level``, what each sets up before its first call, and
the call itself.  The count / allocate / emit loops differ and stay in their modules."""

import ctypes as C

import numpy as np

from . import _native as N


def level32(name, level) -> float:
    """``level`` as the float32 the kernels compare with; a ``ValueError`` in the name of the pass unless it is a
    number that is not NaN in float32."""
    if isinstance(level, (bool, np.bool_)) or not isinstance(level, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}: level must be a number")
    with np.errstate(over="ignore"):
        value = float(np.float32(level))
    if value != value:
        raise ValueError(f"{name}: level must not be NaN")
    return value


def box_pass(volume, symbol, params, lod, box, ids, stream):
    """Checks ``lod``, ``box`` and the id list into ``params`` (the pass's params struct, filled but for them) ->
    ``(lod, scale, dev, call)``.  ``call(words, outputs, *tensors)`` makes one call of the C entry point ``symbol`` and
    returns its header of ``words`` words as ints (coordinates read as int64: signed already); ``outputs(header)``
    builds the outputs struct around the header's address, ``tensors`` are this call's output tensors (None: one it
    does not write).  It synchronises, and holds the uploaded id list for as long as it lives."""
    import torch

    lod = params.lod = volume._check_lod(lod)
    volume._box_params(params, lod, box)
    scale = tuple(float(v) for v in volume.wrapping_buffers[lod].scale_factor)
    handle = volume.prepare()
    dev = torch.device("cuda", volume._rings.device)
    side = torch.cuda.ExternalStream(int(stream), device=dev) if stream is not None else None
    sel = volume._upload_ids(params, ids, dev, side)                   # held until the last call has run
    stream = volume._plane_stream(stream)

    def call(words, outputs, *tensors, sel=sel):
        header = torch.empty(words, dtype=torch.int64, device=dev)
        if side is not None:
            torch.cuda.current_stream(dev).synchronize()               # the allocator's memory may still be in use there
        out = outputs(header.data_ptr())
        N.check(getattr(N.lib(), symbol)(handle, C.byref(params), C.byref(out), C.c_void_p(stream)), symbol)
        if side is not None:
            for t in (*tensors, header):
                if t is not None:
                    t.record_stream(side)
            side.synchronize()
        return [int(v) for v in header.cpu().numpy()]                  # synchronises

    return lod, scale, dev, call
