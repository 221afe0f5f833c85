#!/usr/bin/env python3
"""Time svr_histogram (include/svr.h) on the rings of bench.py's default configuration (C2: 1024^3, three LODs), for
each LOD's full window, on byte rings and on float32 rings: HIP events around runs of back-to-back calls on one stream,
after a warm-up, the median over --repeats runs.  One JSON line per case:

1. the call's bytes per second - read bytes = voxels x element size, plus 4 per voxel with a label filter - and that
   rate as a fraction of a device-to-device hipMemcpyAsync of the same byte count (which reads AND writes that many
   bytes), timed here in the same way;
2. the same for three fills of the finest ring: the synthetic scene, uniform random bytes and all zeros (the contended
   case: every voxel lands in one bin);
3. the only other route to the data: svr_read_region of the same window + np.histogram on the host, wall clock.

usage: python tools/histogram_time.py [--volume-n 1024] [--repeats 9] [--window 0.2] [--bins 256]
"""
import argparse
import ctypes as C
import json
import os
import statistics
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
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--skip-readback", action="store_true", help="leave out route 3 (svr_read_region + np.histogram)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("histogram_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, K = args.volume_n, args.bins
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def histogram_case(vol, lod, what, sel=None, **extra):
        handle = vol.prepare()
        state = N.LodState()
        N.check(lib.svr_get_lod_state(handle, lod, C.byref(state)), "svr_get_lod_state")
        voxels = int(state.shape[0]) * int(state.shape[1]) * int(state.shape[2])
        es = {"uint8": 1, "uint16": 2, "float32": 4}[vol._rings.density_storage]
        nbytes = voxels * (es + (4 if sel is not None else 0))
        counts = torch.empty(K, dtype=torch.int64, device=dev)
        tail = torch.empty(4, dtype=torch.int64, device=dev)
        rng = torch.empty(2, dtype=torch.float32, device=dev)
        hp = N.HistogramParams(lod=lod, lo=0.0, hi=256.0, bins=K)
        if sel is not None:
            hp.selected, hp.selected_count = sel.data_ptr(), sel.numel()
        ho = N.HistogramOutputs(counts.data_ptr(), tail.data_ptr(), rng.data_ptr())
        argv = (handle, C.byref(hp), C.byref(ho), C.c_void_p(stream.cuda_stream))

        med, lo, hi, k = timing.timed(lambda: N.check(lib.svr_histogram(*argv), "svr_histogram"), args.window, args.repeats, k0=10)
        memcpy = nbytes / timing.copy_seconds(nbytes, args.window, args.repeats, k0=10)
        line = {"case": what, "storage": vol._rings.density_storage, "lod": lod, "window": list(state.shape), "bins": K,
                "label_filter": sel is not None, "us_per_call": round(med * 1e6, 2), "us_min_max": [round(lo * 1e6, 2), round(hi * 1e6, 2)],
                "calls_per_run": k, "runs": args.repeats, "read_bytes": nbytes, "GB_per_s": round(nbytes / med / 1e9, 1),
                "memcpy_d2d_GB_per_s": round(memcpy / 1e9, 1), "fraction_of_memcpy": round(nbytes / med / memcpy, 3),
                "considered": int(tail[3]), "largest_bin_share": round(float(counts.max()) / max(int(tail[3]), 1), 4)}
        line.update(extra)
        print(json.dumps(line), flush=True)
        return med

    def readback_case(vol, lod, gpu_seconds):
        """Route 3: what a caller had to do before - read the window back and bin it on the host."""
        handle = vol.prepare()
        state = N.LodState()
        N.check(lib.svr_get_lod_state(handle, lod, C.byref(state)), "svr_get_lod_state")
        shape = [int(v) for v in state.shape]
        ring = [int(v) for v in vol.wrapping_buffers[lod].shape_in_pixels][::-1]
        off = [int(o) % r for o, r in zip(state.offset, ring)]
        if any(o + s > r for o, s, r in zip(off, shape, ring)):        # svr_read_region takes one unwrapped region
            off = [0, 0, 0]
        voxels = shape[0] * shape[1] * shape[2]
        out = np.empty(voxels, np.float32)
        runs = []
        for _ in range(2):
            t0 = time.perf_counter()
            N.check(lib.svr_read_region(handle, lod, N.i3(off), N.i3(shape), out.ctypes.data, None), "svr_read_region")
            t1 = time.perf_counter()
            np.histogram(out, bins=K, range=(0.0, 256.0))
            runs.append((t1 - t0, time.perf_counter() - t1))
        read_s, host_s = (statistics.median(r[i] for r in runs) for i in (0, 1))
        print(json.dumps({"case": "svr_read_region + np.histogram", "storage": vol._rings.density_storage, "lod": lod,
                          "window": shape, "read_region_ms": round(read_s * 1e3, 2), "np_histogram_ms": round(host_s * 1e3, 2),
                          "total_ms": round((read_s + host_s) * 1e3, 2), "svr_histogram_ms": round(gpu_seconds * 1e3, 4),
                          "speedup": round((read_s + host_s) / gpu_seconds, 1)}), flush=True)

    pairs = timing.c2_pairs(n, dev)
    print(json.dumps({"volume_n": n, "bins": K, "device": torch.cuda.get_device_name(0)}), flush=True)
    for storage in ("native", "float32"):
        vol = timing.c2_scene(n, 1920, 1080, "K1", storage, pairs)[1].volume
        torch.cuda.synchronize()
        seconds = [histogram_case(vol, lod, "full window") for lod in range(3)]
        labels = torch.unique(pairs[0][1].reshape(-1)[:: max(1, pairs[0][1].numel() // 100000)])[:16].to(torch.int32).contiguous()
        histogram_case(vol, 0, "full window, 16 labels", sel=labels)
        if not args.skip_readback:
            for lod in range(3):
                readback_case(vol, lod, seconds[lod])
        # the three fills of the finest ring: the whole ring is overwritten from a device array (labels stay)
        ring = [int(v) for v in vol.wrapping_buffers[0].shape_in_pixels]          # numpy order
        histogram_case(vol, 0, "fill: synthetic scene")
        for fill in ("uniform random bytes", "all zeros"):
            values = (torch.randint(0, 256, ring, dtype=torch.uint8, device=dev) if fill.startswith("uniform")
                      else torch.zeros(ring, dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            strides = N.l3([st * values.element_size() for st in values.stride()][::-1])
            N.check(lib.svr_upload_region_device(vol.prepare(), 0, N.i3((0, 0, 0)), N.i3(ring[::-1]), C.c_void_p(values.data_ptr()),
                                                 N.dtype_code(np.dtype("uint8")), strides, None, 0, N.l3((0, 0, 0))),
                    "svr_upload_region_device")
            N.check(lib.svr_publish_uploads(vol.prepare()), "svr_publish_uploads")
            N.check(lib.svr_sync(vol.prepare()), "svr_sync")
            del values
            histogram_case(vol, 0, "fill: " + fill)
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
