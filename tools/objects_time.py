#!/usr/bin/env python3
"""Time svr_objects (include/svr.h) on the rings of bench.py's default configuration (C2: 1024^3, three LODs), for each
LOD's full window, on byte rings and on float32 rings, with and without the label-0 voxels: HIP events around runs of
back-to-back calls on one stream, after a warm-up, the median over --repeats runs.  One JSON line per case, with the
call's bytes per second (read bytes = voxels x (element size + 4 of label)) and, timed here in the same way,

1. a device-to-device hipMemcpyAsync of the same byte count (which reads AND writes that many bytes);
2. the label-filtered svr_histogram (16 ids) of the same window, which reads the same bytes per voxel;
3. the route the call replaces: svr_read_region of density and labels + np.unique / np.bincount on the host, wall clock.

Then a second fill of the finest ring, every voxel its own label (runs of length 1, no two voxels share a record: every
run spills past the LDS table into the global one), on a box of 128 x 256 x 256 voxels against the scene's labels in the
same box.

usage: python tools/objects_time.py [--volume-n 1024] [--repeats 9] [--window 0.2] [--capacity 16384]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--capacity", type=int, default=16384, help="records of the table (the scene has 4096 labels)")
    ap.add_argument("--readback-lods", default="0,1,2", help="LODs on which route 3 is timed ('' for none)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("objects_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)
    readback_lods = [int(v) for v in args.readback_lods.split(",") if v != ""]

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=5)

    def window_of(vol, lod):
        state = N.LodState()
        N.check(lib.svr_get_lod_state(vol.prepare(), lod, C.byref(state)), "svr_get_lod_state")
        return state

    def histogram_seconds(vol, lod, sel, box):
        counts = torch.empty(256, dtype=torch.int64, device=dev)
        tail = torch.empty(4, dtype=torch.int64, device=dev)
        hp = N.HistogramParams(lod=lod, lo=0.0, hi=256.0, bins=256)
        hp.selected, hp.selected_count = sel.data_ptr(), sel.numel()
        if box is not None:
            hp.use_box = 1
            hp.box_off[:], hp.box_shape[:] = box
        ho = N.HistogramOutputs(counts.data_ptr(), tail.data_ptr(), None)
        argv = (vol.prepare(), C.byref(hp), C.byref(ho), C.c_void_p(stream.cuda_stream))

        return timed(lambda: N.check(lib.svr_histogram(*argv), "svr_histogram"))[0]

    def objects_case(vol, lod, what, sel16, background, capacity, box=None, comparators=True):
        state = window_of(vol, lod)
        shape = [int(v) for v in state.shape] if box is None else list(box[1])
        voxels = shape[0] * shape[1] * shape[2]
        es = {"uint8": 1, "uint16": 2, "float32": 4}[vol._rings.density_storage]
        nbytes = voxels * (es + 4)
        records = torch.empty((capacity, 12), dtype=torch.int64, device=dev)
        header = torch.empty(8, dtype=torch.int64, device=dev)
        op = N.ObjectsParams(lod=lod, capacity=capacity, ignore_zero=0 if background else 1)
        if box is not None:
            op.use_box = 1
            op.box_off[:], op.box_shape[:] = box
        oo = N.ObjectsOutputs(records.data_ptr(), header.data_ptr())
        argv = (vol.prepare(), C.byref(op), C.byref(oo), C.c_void_p(stream.cuda_stream))

        med, lo, hi, k = timed(lambda: N.check(lib.svr_objects(*argv), "svr_objects"))
        head = [int(v) for v in header.cpu().numpy()]
        line = {"case": what, "storage": vol._rings.density_storage, "lod": lod, "shape": shape, "background": background,
                "capacity": capacity, "us_per_call": round(med * 1e6, 2), "us_min_max": [round(lo * 1e6, 2), round(hi * 1e6, 2)],
                "calls_per_run": k, "runs": args.repeats, "read_bytes": nbytes, "GB_per_s": round(nbytes / med / 1e9, 1),
                "objects": head[0], "considered": head[1], "overflow": head[2], "dropped_label_0": head[3]}
        if comparators:
            memcpy = timing.copy_seconds(nbytes, args.window, args.repeats, k0=5)
            hist = histogram_seconds(vol, lod, sel16, box)
            line.update({"memcpy_d2d_us": round(memcpy * 1e6, 2), "ratio_to_memcpy": round(med / memcpy, 2),
                         "histogram_16_labels_us": round(hist * 1e6, 2), "ratio_to_histogram": round(med / hist, 2)})
        print(json.dumps(line), flush=True)
        del records, header
        return med

    def readback_case(vol, lod, gpu_seconds):
        """Route 3: read density and labels of the window back and group them on the host."""
        state = window_of(vol, lod)
        shape = [int(v) for v in state.shape]
        ring = [int(v) for v in vol.wrapping_buffers[lod].shape_in_pixels][::-1]
        off = [int(o) % r for o, r in zip(state.offset, ring)]
        if any(o + s > r for o, s, r in zip(off, shape, ring)):        # svr_read_region takes one unwrapped region
            off = [0, 0, 0]
        voxels = shape[0] * shape[1] * shape[2]
        den, lab = np.empty(voxels, np.float32), np.empty(voxels, np.uint32)
        t0 = time.perf_counter()
        N.check(lib.svr_read_region(vol.prepare(), lod, N.i3(off), N.i3(shape), den.ctypes.data, lab.ctypes.data), "svr_read_region")
        t1 = time.perf_counter()
        ids, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
        sums = np.bincount(inverse.reshape(-1), weights=den, minlength=ids.size)
        t2 = time.perf_counter()
        print(json.dumps({"case": "svr_read_region + np.unique / np.bincount (voxels and mean only)", "storage": vol._rings.density_storage,
                          "lod": lod, "window": shape, "read_region_ms": round((t1 - t0) * 1e3, 2), "numpy_ms": round((t2 - t1) * 1e3, 2),
                          "total_ms": round((t2 - t0) * 1e3, 2), "objects": int(ids.size), "svr_objects_ms": round(gpu_seconds * 1e3, 4),
                          "speedup": round((t2 - t0) / gpu_seconds, 1), "checksum": float(sums.sum()) + int(counts.sum())}), flush=True)

    pairs = timing.c2_pairs(n, dev)
    print(json.dumps({"volume_n": n, "device": torch.cuda.get_device_name(0)}), flush=True)
    sel16 = torch.unique(pairs[0][1].reshape(-1)[:: max(1, pairs[0][1].numel() // 100000)])[:16].to(torch.int32).contiguous()
    for storage in ("native", "float32"):
        vol = timing.c2_scene(n, 1920, 1080, "K1", storage, pairs)[1].volume
        torch.cuda.synchronize()
        for lod in range(3):
            seconds = objects_case(vol, lod, "full window", sel16, True, args.capacity)
            objects_case(vol, lod, "full window", sel16, False, args.capacity, comparators=False)
            if lod in readback_lods:
                readback_case(vol, lod, seconds)
        # the spill path: the same box of the finest ring with the scene's labels, then with every voxel its own label
        state = window_of(vol, 0)
        shape = [min(int(state.shape[0]), 256), min(int(state.shape[1]), 256), min(int(state.shape[2]), 128)]
        box = ([int(v) for v in state.offset], shape)
        own_capacity = 1 << max(12, (2 * shape[0] * shape[1] * shape[2] - 1).bit_length())       # load <= 0.5
        objects_case(vol, 0, "box, the scene's labels", sel16, True, args.capacity, box=box)
        objects_case(vol, 0, "box, the scene's labels, the large table", sel16, True, min(own_capacity, N.OBJECTS_MAX_CAPACITY), box=box,
                     comparators=False)
        ring = [int(v) for v in vol.wrapping_buffers[0].shape_in_pixels]          # numpy order
        values = torch.randint(0, 256, ring, dtype=torch.uint8, device=dev)
        own = (torch.arange(values.numel(), dtype=torch.int64, device=dev) + 1).to(torch.int32).reshape(ring)
        torch.cuda.synchronize()
        N.check(lib.svr_upload_region_device(vol.prepare(), 0, N.i3((0, 0, 0)), N.i3(ring[::-1]), C.c_void_p(values.data_ptr()),
                                             N.dtype_code(np.dtype("uint8")), N.l3([st for st in values.stride()][::-1]),
                                             C.c_void_p(own.data_ptr()), N.dtype_code(np.dtype("uint32")),
                                             N.l3([st * 4 for st in own.stride()][::-1])), "svr_upload_region_device")
        N.check(lib.svr_publish_uploads(vol.prepare()), "svr_publish_uploads")
        N.check(lib.svr_sync(vol.prepare()), "svr_sync")
        del values, own
        objects_case(vol, 0, "box, every voxel its own label", sel16, True, min(own_capacity, N.OBJECTS_MAX_CAPACITY), box=box,
                     comparators=False)
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
