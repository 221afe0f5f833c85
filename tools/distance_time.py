#!/usr/bin/env python3
"""Time svr_distance (include/svr.h) on a box of up to 512^3 voxels of the finest ring of bench.py's default
configuration (C2: 1024^3, three LODs), on byte rings and on float32 rings: a level set at the median value, one at the
98th percentile, every label but 0, a level below every value with the border on (the solid worst case: every column as
long as the box and a deepest point in its middle), and the 98th-percentile level inverted (most voxels are targets).  HIP
events around runs of back-to-back calls on one stream, after a warm-up, the median over --repeats runs (timing.timed),
for the count-only call and for the full call.  One JSON line per case, beside three references timed in the same run:

1. the full svr_components call (6-connectivity, exact capacities) on the same box and inside set;
2. a device-to-device copy of the bytes the result occupies (4 per voxel): the passes cannot beat a small multiple of it;
3. the route a user has today: svr_read_region of the box + scipy.ndimage.distance_transform_edt, wall clock (once per
   storage, on the median level set; scipy runs on a --cpu-box^3 corner of the box and is scaled by voxels, as the line
   notes).

usage: python tools/distance_time.py [--volume-n 1024] [--box 512] [--repeats 9] [--window 0.2] [--cpu-box 256] [--no-cpu]
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
    ap.add_argument("--box", type=int, default=512, help="edge of the box (cut to the window)")
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--storages", default="native,float32")
    ap.add_argument("--cpu-box", type=int, default=256, help="edge of the corner of the box scipy runs on")
    ap.add_argument("--no-cpu", action="store_true", help="leave the read-back + scipy route out")
    ap.add_argument("--no-components", action="store_true", help="leave the svr_components reference out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("distance_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=2)          # (the warm-up also allocates the scratch)

    def distance_call(vol, box, level, invert, border, d2, header):
        dp = N.DistanceParams(lod=0, use_box=1, invert=invert, border=border)
        dp.box_off[:], dp.box_shape[:] = box
        if level is not None:
            dp.mode, dp.level = N.COMPONENTS_LEVEL, level
        else:
            dp.mode, dp.ignore_zero = N.COMPONENTS_LABELS, 1
        do = N.DistanceOutputs(None if d2 is None else d2.data_ptr(), 0 if d2 is None else d2.numel(), header.data_ptr())
        argv = (vol.prepare(), C.byref(dp), C.byref(do), C.c_void_p(stream.cuda_stream))

        def one():
            N.check(lib.svr_distance(*argv), "svr_distance")

        one.keep = (dp, do)
        return one

    def components_seconds(vol, box, level, voxels):
        header = torch.empty(16, dtype=torch.int64, device=dev)

        def call(ids, records):
            cp = N.ComponentsParams(lod=0, use_box=1, connectivity=6)
            cp.box_off[:], cp.box_shape[:] = box
            if level is not None:
                cp.mode, cp.level = N.COMPONENTS_LEVEL, level
            else:
                cp.mode, cp.ignore_zero = N.COMPONENTS_LABELS, 1
            co = N.ComponentsOutputs(None if ids is None else ids.data_ptr(), 0 if ids is None else ids.numel(),
                                     None if records is None else records.data_ptr(), 0 if records is None else records.shape[0], header.data_ptr())
            argv = (vol.prepare(), C.byref(cp), C.byref(co), C.c_void_p(stream.cuda_stream))
            one = lambda: N.check(lib.svr_components(*argv), "svr_components")
            one.keep = (cp, co)
            return one

        call(None, None)()
        count = int(header.cpu().numpy()[0])
        ids = torch.empty(voxels, dtype=torch.int32, device=dev)
        records = torch.empty((max(count, 1), N.COMPONENT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
        return timed(call(ids, records))[0]

    def cpu_route(vol, box, level):
        """svr_read_region of the box + scipy's EDT of a corner of it -> (read seconds, EDT seconds scaled to the box, note)."""
        from scipy import ndimage

        ring = [int(v) for v in vol.wrapping_buffers[0].shape_in_pixels][::-1]
        off = [int(o) % r for o, r in zip(box[0], ring)]
        shape = list(box[1])
        if any(o + s > r for o, s, r in zip(off, shape, ring)):        # svr_read_region takes one unwrapped region: the same bytes from slot 0
            off = [0, 0, 0]
        voxels = shape[0] * shape[1] * shape[2]
        den, lab = np.empty(voxels, np.float32), np.empty(voxels, np.uint32)
        t0 = time.perf_counter()
        N.check(lib.svr_read_region(vol.prepare(), 0, N.i3(off), N.i3(shape), den.ctypes.data, lab.ctypes.data), "svr_read_region")
        t1 = time.perf_counter()
        e = min(args.cpu_box, *shape)
        inside = (den.reshape(shape[::-1])[:e, :e, :e] >= np.float32(level)).copy()
        t2 = time.perf_counter()
        ndimage.distance_transform_edt(inside)
        edt = time.perf_counter() - t2
        return t1 - t0, edt * voxels / float(e ** 3), f"a {e}^3 corner of the box, scaled by voxels"

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
        # the median value and the 98th percentile as the levels
        hist = vol.histogram(lod=0, bins=256, range=(0.0, 256.0), box=numpy_box)
        cum = torch.cumsum(hist.counts, 0)
        median = float(int(torch.searchsorted(cum, cum[-1] // 2)) + 1)
        high = float(int(torch.searchsorted(cum, cum[-1] * 98 // 100)) + 1)
        header = torch.empty(16, dtype=torch.int64, device=dev)
        d2 = torch.empty(voxels, dtype=torch.int32, device=dev)
        copy_s = timing.copy_seconds(voxels * 4, args.window, args.repeats, 3)
        typical = None
        for what, level, invert, border in (("level, median", median, 0, 1), ("level, 98th percentile", high, 0, 1), ("every label but 0", None, 0, 1),
                                            ("solid, border", -1.0, 0, 1), ("level, 98th percentile, inverted", high, 1, 0)):
            count_s, c_lo, c_hi, c_k = timed(distance_call(vol, box, level, invert, border, None, header))
            full_s, f_lo, f_hi, f_k = timed(distance_call(vol, box, level, invert, border, d2, header))
            head = [int(v) for v in header.cpu().numpy()]
            assert head[2] == voxels, head
            if typical is None:
                typical = full_s
            line = {
                "case": what, "storage": vol._rings.density_storage, "box": shape, "voxels": voxels, "level": level, "invert": invert, "border": border,
                "targets": head[0], "inside_voxels": head[1], "max_squared": head[3], "far": head[15],
                "count_ms": round(count_s * 1e3, 4), "count_ms_min_max": [round(c_lo * 1e3, 4), round(c_hi * 1e3, 4)], "count_calls_per_run": c_k,
                "full_ms": round(full_s * 1e3, 4), "full_ms_min_max": [round(f_lo * 1e3, 4), round(f_hi * 1e3, 4)], "full_calls_per_run": f_k,
                "runs": args.repeats, "copy_of_result_bytes_ms": round(copy_s * 1e3, 4), "full_over_copy": round(full_s / copy_s, 2),
                "full_over_first_case": round(full_s / typical, 2)}
            if not args.no_components and what != "solid, border":
                comp_s = components_seconds(vol, box, level, voxels)
                line.update({"components_full_ms": round(comp_s * 1e3, 4), "full_over_components": round(full_s / comp_s, 2)})
            if not args.no_cpu and what == "level, median":
                read_s, edt_s, note = cpu_route(vol, box, level)
                line.update({"read_region_ms": round(read_s * 1e3, 1), "scipy_edt_ms": round(edt_s * 1e3, 1), "scipy_on": note,
                             "today_over_full": round((read_s + edt_s) / full_s, 1)})
            print(json.dumps(line), flush=True)
        del d2
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
