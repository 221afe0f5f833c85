#!/usr/bin/env python3
"""Time svr_split (include/svr.h) on the squared distances of a box of up to 512^3 voxels of the finest ring of
bench.py's default configuration (C2: 1024^3, three LODs, byte rings): a level set at the median value and one at the
98th percentile, under 6- and 26-connectivity, merge_squared = 1.  HIP events around runs of back-to-back calls on one
stream, after a warm-up, the median over --repeats runs (timing.timed), for the count-only call and for the full call
(exact capacities).  One JSON line per case, beside three references timed in the same run:

1. the full svr_components call on the same inside set and connectivity: a union-find pass, a scan and an emit too;
2. the full svr_distance call that wrote the field;
3. a device-to-device copy of the field's bytes (4 per voxel).

And once, the route a user has today: the field copied to the host plus the numpy restatement of the call
(tests/split_twin.py) on a 64^3 corner of it, wall clock, SCALED by voxels to the box, as the line says.

usage: python tools/split_time.py [--volume-n 1024] [--box 512] [--repeats 9] [--window 0.2] [--no-cpu]
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
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--box", type=int, default=512, help="edge of the box (cut to the window)")
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--merge-squared", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true", help="leave the copy-to-host + numpy route out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("split_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=2)          # (the warm-up also allocates the scratch)

    def ms(t):
        return {"ms": round(t[0] * 1e3, 4), "ms_min_max": [round(t[1] * 1e3, 4), round(t[2] * 1e3, 4)], "calls_per_run": t[3]}

    pairs = timing.c2_pairs(n, dev)
    print(json.dumps({"volume_n": n, "device": torch.cuda.get_device_name(0)}), flush=True)
    vol = timing.c2_scene(n, 1920, 1080, "K1", "native", pairs)[1].volume
    torch.cuda.synchronize()
    handle = vol.prepare()
    state = N.LodState()
    N.check(lib.svr_get_lod_state(handle, 0, C.byref(state)), "svr_get_lod_state")
    shape = [min(int(s), args.box) for s in state.shape]
    box = ([int(v) for v in state.offset], shape)
    voxels = shape[0] * shape[1] * shape[2]
    numpy_box = (tuple(box[0][::-1]), tuple(o + s for o, s in zip(box[0][::-1], shape[::-1])))
    hist = vol.histogram(lod=0, bins=256, range=(0.0, 256.0), box=numpy_box)
    cum = torch.cumsum(hist.counts, 0)
    median = float(int(torch.searchsorted(cum, cum[-1] // 2)) + 1)
    high = float(int(torch.searchsorted(cum, cum[-1] * 98 // 100)) + 1)
    header = torch.empty(16, dtype=torch.int64, device=dev)
    d2 = torch.empty(voxels, dtype=torch.int32, device=dev)
    ids = torch.empty(voxels, dtype=torch.int32, device=dev)
    copy_s = timing.copy_seconds(voxels * 4, args.window, args.repeats, 3)
    cpu_done = args.no_cpu

    for what, level in (("level, median", median), ("level, high", high)):
        dp = N.DistanceParams(lod=0, use_box=1, mode=N.COMPONENTS_LEVEL, level=level, border=1)
        dp.box_off[:], dp.box_shape[:] = box
        do = N.DistanceOutputs(d2.data_ptr(), voxels, header.data_ptr())
        dist_argv = (handle, C.byref(dp), C.byref(do), C.c_void_p(stream.cuda_stream))
        dist = timed(lambda: N.check(lib.svr_distance(*dist_argv), "svr_distance"))
        dist_head = [int(v) for v in header.cpu().numpy()]
        assert dist_head[2] == voxels, dist_head
        for connectivity in (6, 26):
            cp = N.ComponentsParams(lod=0, use_box=1, connectivity=connectivity, mode=N.COMPONENTS_LEVEL, level=level)
            cp.box_off[:], cp.box_shape[:] = box
            co = N.ComponentsOutputs(None, 0, None, 0, header.data_ptr())
            N.check(lib.svr_components(handle, C.byref(cp), C.byref(co), C.c_void_p(stream.cuda_stream)), "svr_components")
            comp_count = int(header.cpu().numpy()[0])
            comp_records = torch.empty((max(comp_count, 1), N.COMPONENT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
            co = N.ComponentsOutputs(ids.data_ptr(), voxels, comp_records.data_ptr(), comp_records.shape[0], header.data_ptr())
            comp_argv = (handle, C.byref(cp), C.byref(co), C.c_void_p(stream.cuda_stream))
            comp = timed(lambda: N.check(lib.svr_components(*comp_argv), "svr_components"))
            largest = int(comp_records.view(torch.int64)[:comp_count, 1].max()) if comp_count else 0

            sp = N.SplitParams(height=d2.data_ptr(), connectivity=connectivity, merge_squared=args.merge_squared)
            sp.n[:] = shape
            so = N.SplitOutputs(None, 0, None, 0, header.data_ptr())
            count_argv = (handle, C.byref(sp), C.byref(so), C.c_void_p(stream.cuda_stream))
            count = timed(lambda: N.check(lib.svr_split(*count_argv), "svr_split"))
            head = [int(v) for v in header.cpu().numpy()]
            records = torch.empty((max(head[0], 1), N.SPLIT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
            so_full = N.SplitOutputs(ids.data_ptr(), voxels, records.data_ptr(), records.shape[0], header.data_ptr())
            full_argv = (handle, C.byref(sp), C.byref(so_full), C.c_void_p(stream.cuda_stream))
            full = timed(lambda: N.check(lib.svr_split(*full_argv), "svr_split"))
            head = [int(v) for v in header.cpu().numpy()]
            assert head[2] == voxels and head[3] == head[0], head
            r64 = records.view(torch.int64)[:head[0]]
            line = {"case": what, "connectivity": connectivity, "merge_squared": args.merge_squared, "box": shape, "voxels": voxels, "level": level,
                    "inside_voxels": head[1], "basins": head[4], "regions": head[0], "components": comp_count, "largest_component": largest,
                    "largest_region": int(r64[:, 1].max()) if head[0] else 0, "runs": args.repeats,
                    "count": ms(count), "full": ms(full), "components_full": ms(comp), "distance_full": ms(dist),
                    "copy_of_field_bytes_ms": round(copy_s * 1e3, 4),
                    "full_over_components_full": round(full[0] / comp[0], 2), "full_over_distance_full": round(full[0] / dist[0], 2),
                    "full_over_copy": round(full[0] / copy_s, 2)}
            print(json.dumps(line), flush=True)
            if not cpu_done:                                           # once: what a user does today, on this field
                from split_twin import split_twin

                cpu_done = True
                t0 = time.perf_counter()
                host = d2.reshape(shape[::-1]).cpu().numpy()
                t1 = time.perf_counter()
                e = min(64, *shape)
                corner = np.ascontiguousarray(host[:e, :e, :e])
                t2 = time.perf_counter()
                twin = split_twin(corner, connectivity, args.merge_squared)
                twin_s = time.perf_counter() - t2
                scaled = twin_s * voxels / float(e ** 3)
                print(json.dumps({"case": "field copied to the host + numpy restatement (tests/split_twin.py)", "of": what, "connectivity": connectivity,
                                  "copy_to_host_ms": round((t1 - t0) * 1e3, 1), "twin_corner": [e, e, e], "twin_corner_ms": round(twin_s * 1e3, 1),
                                  "twin_corner_regions": twin["header"][0],
                                  "twin_ms_SCALED_by_voxels_to_the_box": round(scaled * 1e3, 1),
                                  "today_over_full_SCALED": round(((t1 - t0) + scaled) / full[0], 1)}), flush=True)
            del records, comp_records
    vol.close()


if __name__ == "__main__":
    main()
