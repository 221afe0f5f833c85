#!/usr/bin/env python3
"""Time svr_contacts (include/svr.h) on the rings of bench.py's default configuration (C2: 1024^3, three LODs), for each
LOD's full window and for a box of 256 x 256 x 128 voxels of the finest one, on byte rings and on float32 rings, with
and without the faces of label 0: HIP events around runs of back-to-back calls on one stream, after a warm-up, the
median over --repeats runs (tools/timing.py).  One JSON line per case, and, timed in the same run in the same way,

1. svr_objects on the same window or box;
2. a device-to-device hipMemcpyAsync of the bytes svr_objects reads there (voxels x (element size + 4 of label)),
   which reads AND writes that many bytes.

Once per ring type, on --readback-lod, the route the call replaces: svr_read_region of density and labels, then the
numpy restatement of the call (tests/contacts_twin.py: three shifted comparisons and a sort of the pairs), wall clock.

usage: python tools/contacts_time.py [--volume-n 1024] [--repeats 9] [--window 0.2] [--capacity 65536]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--capacity", type=int, default=65536, help="records of the table (the scene has 4096 labels)")
    ap.add_argument("--readback-lod", type=int, default=2, help="the LOD on which the read-back route is timed (-1: none; 2: the smallest window, 19 M voxels)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from contacts_twin import contacts_twin
    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("contacts_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=5)

    def window_of(vol, lod):
        state = N.LodState()
        N.check(lib.svr_get_lod_state(vol.prepare(), lod, C.byref(state)), "svr_get_lod_state")
        return state

    def pass_seconds(vol, symbol, params_type, outputs_type, words, lod, background, box):
        records = torch.empty((args.capacity, words), dtype=torch.int64, device=dev)
        header = torch.empty(8, dtype=torch.int64, device=dev)
        p = params_type(lod=lod, capacity=args.capacity, ignore_zero=0 if background else 1)
        if box is not None:
            p.use_box = 1
            p.box_off[:], p.box_shape[:] = box
        o = outputs_type(records.data_ptr(), header.data_ptr())
        argv = (vol.prepare(), C.byref(p), C.byref(o), C.c_void_p(stream.cuda_stream))
        call = getattr(lib, symbol)
        med, lo, hi, k = timed(lambda: N.check(call(*argv), symbol))
        return med, lo, hi, k, [int(v) for v in header.cpu().numpy()]

    def contacts_case(vol, lod, what, background, box=None, comparators=True):
        state = window_of(vol, lod)
        shape = [int(v) for v in state.shape] if box is None else list(box[1])
        voxels = shape[0] * shape[1] * shape[2]
        es = {"uint8": 1, "uint16": 2, "float32": 4}[vol._rings.density_storage]
        nbytes = voxels * (es + 4)
        med, lo, hi, k, head = pass_seconds(vol, "svr_contacts", N.ContactsParams, N.ContactsOutputs, N.CONTACT_RECORD_BYTES // 8, lod, background, box)
        line = {"case": what, "storage": vol._rings.density_storage, "lod": lod, "shape": shape, "background": background,
                "capacity": args.capacity, "us_per_call": round(med * 1e6, 2), "us_min_max": [round(lo * 1e6, 2), round(hi * 1e6, 2)],
                "calls_per_run": k, "runs": args.repeats, "label_bytes": voxels * 4, "label_GB_per_s": round(voxels * 4 / med / 1e9, 1),
                "pairs": head[0], "faces": head[1], "overflow": head[2], "dropped_label_0": head[3], "voxels": head[7]}
        if comparators:
            obj = pass_seconds(vol, "svr_objects", N.ObjectsParams, N.ObjectsOutputs, N.OBJECT_RECORD_BYTES // 8, lod, background, box)[0]
            memcpy = timing.copy_seconds(nbytes, args.window, args.repeats, k0=5)
            line.update({"svr_objects_us": round(obj * 1e6, 2), "ratio_to_objects": round(med / obj, 2), "objects_read_bytes": nbytes,
                         "memcpy_d2d_us": round(memcpy * 1e6, 2), "ratio_to_memcpy": round(med / memcpy, 2)})
        print(json.dumps(line), flush=True)
        return med

    def readback_case(vol, lod, gpu_seconds):
        """The route a user has today: read density and labels of the window back, then the numpy restatement."""
        state = window_of(vol, lod)
        shape = [int(v) for v in state.shape]
        ring = [int(v) for v in vol.wrapping_buffers[lod].shape_in_pixels][::-1]
        off = [int(o) % r for o, r in zip(state.offset, ring)]
        if any(o + s > r for o, s, r in zip(off, shape, ring)):        # svr_read_region takes one unwrapped region
            off = [0, 0, 0]
        den, lab = np.empty(shape[::-1], np.float32), np.empty(shape[::-1], np.uint32)
        t0 = time.perf_counter()
        N.check(lib.svr_read_region(vol.prepare(), lod, N.i3(off), N.i3(shape), den.ctypes.data, lab.ctypes.data), "svr_read_region")
        t1 = time.perf_counter()
        # the block that was read is its own ring here: the pairs and their faces are those of the window
        twin = contacts_twin(dict(density=den, labels=lab, offset=(0, 0, 0), shape=tuple(shape)), integer=vol._rings.density_storage != "float32")
        t2 = time.perf_counter()
        print(json.dumps({"case": "svr_read_region + numpy restatement (tests/contacts_twin.py)", "storage": vol._rings.density_storage,
                          "lod": lod, "window": shape, "read_region_ms": round((t1 - t0) * 1e3, 2), "numpy_ms": round((t2 - t1) * 1e3, 2),
                          "total_ms": round((t2 - t0) * 1e3, 2), "pairs": twin["header"][0], "faces": twin["header"][1],
                          "svr_contacts_ms": round(gpu_seconds * 1e3, 4), "speedup": round((t2 - t0) / gpu_seconds, 1)}), flush=True)

    pairs = timing.c2_pairs(n, dev)
    print(json.dumps({"volume_n": n, "device": torch.cuda.get_device_name(0)}), flush=True)
    for storage in ("native", "float32"):
        vol = timing.c2_scene(n, 1920, 1080, "K1", storage, pairs)[1].volume
        torch.cuda.synchronize()
        for lod in range(3):
            seconds = contacts_case(vol, lod, "full window", True)
            contacts_case(vol, lod, "full window", False, comparators=False)
            if lod == args.readback_lod:
                readback_case(vol, lod, seconds)
        state = window_of(vol, 0)
        shape = [min(int(state.shape[0]), 256), min(int(state.shape[1]), 256), min(int(state.shape[2]), 128)]
        contacts_case(vol, 0, "box", True, box=([int(v) for v in state.offset], shape))
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
