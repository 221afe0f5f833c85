#!/usr/bin/env python3
"""Time svr_nearest (include/svr.h) on a box of up to 512^3 voxels of the finest ring of bench.py's default configuration
(C2: 1024^3, three LODs) on byte rings: a level set at the median value and one at the 98th percentile, and every label
but 0, each with ``invert`` off and on, and each with the label array written and left out (NULL).  HIP events around
runs of back-to-back calls on one stream, after a warm-up, the median over --repeats runs (timing.timed), for the
count-only call and for the full call.  One JSON line per case, beside two references timed in the same run:

1. the full svr_distance call with border = 0 on the same box and parameters: the yardstick, as svr_nearest computes the
   same d2 and writes two dense arrays and three owner planes more;
2. a device-to-device copy of the bytes one of the result's arrays occupies (4 per voxel: 512 MiB for 512^3).

usage: python tools/nearest_time.py [--volume-n 1024] [--box 512] [--repeats 9] [--window 0.2] [--storages native]
"""
import argparse
import ctypes as C
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--box", type=int, default=512, help="edge of the box (cut to the window)")
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--storages", default="native")
    args = ap.parse_args()

    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("nearest_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=2)          # (the warm-up also allocates the scratch)

    def fill(p, box, level, invert):
        p.lod, p.use_box, p.invert = 0, 1, invert
        p.box_off[:], p.box_shape[:] = box
        if level is not None:
            p.mode, p.level = N.COMPONENTS_LEVEL, level
        else:
            p.mode, p.ignore_zero = N.COMPONENTS_LABELS, 1
        return p

    def nearest_call(vol, box, level, invert, arrays, header):
        p = fill(N.NearestParams(), box, level, invert)
        out = N.NearestOutputs(*[None if t is None else t.data_ptr() for t in arrays], 0 if arrays[0] is None else arrays[0].numel(), header.data_ptr())
        argv = (vol.prepare(), C.byref(p), C.byref(out), C.c_void_p(stream.cuda_stream))

        def one():
            N.check(lib.svr_nearest(*argv), "svr_nearest")

        one.keep = (p, out)
        return one

    def distance_call(vol, box, level, invert, d2, header):
        p = fill(N.DistanceParams(border=0), box, level, invert)
        out = N.DistanceOutputs(d2.data_ptr(), d2.numel(), header.data_ptr())
        argv = (vol.prepare(), C.byref(p), C.byref(out), C.c_void_p(stream.cuda_stream))

        def one():
            N.check(lib.svr_distance(*argv), "svr_distance")

        one.keep = (p, out)
        return one

    pairs = timing.c2_pairs(n, dev)
    print(json.dumps({"volume_n": n, "device": torch.cuda.get_device_name(0)}), flush=True)
    for storage in args.storages.split(","):
        vol = timing.c2_scene(n, 1920, 1080, "K1", storage, pairs)[1].volume
        torch.cuda.synchronize()
        state = N.LodState()
        N.check(lib.svr_get_lod_state(vol.prepare(), 0, C.byref(state)), "svr_get_lod_state")
        shape = [min(int(s), args.box) for s in state.shape]
        box = ([int(v) for v in state.offset], shape)
        voxels = shape[0] * shape[1] * shape[2]
        numpy_box = (tuple(box[0][::-1]), tuple(o + s for o, s in zip(box[0][::-1], shape[::-1])))
        hist = vol.histogram(lod=0, bins=256, range=(0.0, 256.0), box=numpy_box)
        cum = torch.cumsum(hist.counts, 0)
        median = float(int(torch.searchsorted(cum, cum[-1] // 2)) + 1)
        high = float(int(torch.searchsorted(cum, cum[-1] * 98 // 100)) + 1)
        header = torch.empty(16, dtype=torch.int64, device=dev)
        d2, index, label = (torch.empty(voxels, dtype=torch.int32, device=dev) for _ in range(3))
        copy_s = timing.copy_seconds(voxels * 4, args.window, args.repeats, 3)
        for what, level in (("level, median", median), ("level, 98th percentile", high), ("every label but 0", None)):
            for invert in (0, 1):
                dist_s, d_lo, d_hi, d_k = timed(distance_call(vol, box, level, invert, d2, header))
                dist_head = [int(v) for v in header.cpu().numpy()]
                count_s, c_lo, c_hi, c_k = timed(nearest_call(vol, box, level, invert, (None, None, None), header))
                for with_label in (1, 0):
                    full_s, f_lo, f_hi, f_k = timed(nearest_call(vol, box, level, invert, (d2, index, label if with_label else None), header))
                    head = [int(v) for v in header.cpu().numpy()]
                    assert head == dist_head and head[2] == voxels, (head, dist_head)
                    print(json.dumps({
                        "case": what, "storage": vol._rings.density_storage, "box": shape, "voxels": voxels, "level": level, "invert": invert,
                        "label": with_label, "targets": head[0], "inside_voxels": head[1], "max_squared": head[3], "far": head[15],
                        "count_ms": round(count_s * 1e3, 4), "count_ms_min_max": [round(c_lo * 1e3, 4), round(c_hi * 1e3, 4)], "count_calls_per_run": c_k,
                        "full_ms": round(full_s * 1e3, 4), "full_ms_min_max": [round(f_lo * 1e3, 4), round(f_hi * 1e3, 4)], "full_calls_per_run": f_k,
                        "distance_full_ms": round(dist_s * 1e3, 4), "distance_ms_min_max": [round(d_lo * 1e3, 4), round(d_hi * 1e3, 4)],
                        "distance_calls_per_run": d_k, "full_over_distance": round(full_s / dist_s, 2),
                        "runs": args.repeats, "copy_of_one_array_ms": round(copy_s * 1e3, 4), "full_over_copy": round(full_s / copy_s, 2)}), flush=True)
        del d2, index, label
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
