#!/usr/bin/env python3
"""Time svr_slice (cross-section views, include/svr.h) at 1920 x 1080 on the BASELINE config 2 scene (1024^3, the
bench's workload) with byte rings and with float32 rings: z-, y-, x-normal and one oblique plane through the camera's
focus at 1 voxel per pixel, with the default routing of the micro-block copy of LOD 0, rows only (variant bit 8) and
the copy always (bit 9).  svr_slice is called through the C ABI with prebuilt argument structs, as
tools/outline_time.py calls svr_outline.  Two numbers per case, each the median of --boxes windows of --calls calls
after a warm-up (timing.held, tools/timing.py):
  call_us  HIP events around back-to-back calls: what a caller that issues slices one after another sees (host
           enqueue and device both count, whichever is slower);
  gpu_us   the same calls enqueued while the stream is held by a sleep kernel (calibrated to outlast the enqueue), the
           events recorded after it: the device drains a full queue, so this is GPU time per slice (kernel + the
           dispatch gap between kernels), free of host pacing.
plus the bytes written (all six planes), their share of 6.3 TB/s at gpu_us (what a streaming float4 copy reaches),
and a lower bound on the bytes read (each distinct texel once: density element + label).  Kernel durations proper
come from a separate traced run, whose dispatches --trace-db attributes to the cases by their order (per ring type:
one dispatch that allocates the outputs, then per case 20 warm-up + 2 x boxes x calls timed dispatches):

usage: python tools/slice_time.py [--calls 200] [--boxes 5] [--volume-n 1024]
       rocprofv3 --kernel-trace -d DIR -o slice -- python tools/slice_time.py --calls 100 --boxes 2
       python tools/slice_time.py --calls 100 --boxes 2 --trace-db DIR/slice_results.db     (no GPU needed)
"""
import argparse
import json
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12
PLANES = (("z", None), ("y", None), ("x", None), ("oblique", ((0.8, 0.6, 0.0), (-0.36, 0.48, 0.8))))


def texels_read(vol, origin, u, v, W, H):
    """Distinct (LOD, voxel) pairs the slice reads, from the definition in svr.h (host float32)."""
    f32 = np.float32
    size = vol._volume_dimensions.astype(f32)
    ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    fx, fy = (xs + f32(0.5)) - f32(0.5 * W), (ys + f32(0.5)) - f32(0.5 * H)
    m = vol.world.inverse_matrix.astype(f32)
    p = [(f32(origin[k]) + fx * f32(u[k])) + fy * f32(v[k]) for k in range(3)]
    d = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] for k in range(3)]
    d = [((d[k] + f32(0.5)) / size[k]) * size[k] for k in range(3)]
    todo = np.ones(d[0].shape, bool)
    for k in range(3):
        todo &= (d[k] >= 0) & (d[k] < size[k])
    total = 0
    for b in vol.wrapping_buffers:
        st = b.uniform_buffer.data
        off, shp = st["current_logical_offset_in_pixels"], st["current_logical_shape_in_pixels"]
        scale = b.scale_factor[::-1]                                  # shader order
        ic = [np.where(todo, d[k] * f32(scale[k]), 0).astype(np.int64) for k in range(3)]
        inb = todo.copy()
        for k in range(3):
            inb &= (off[k] <= ic[k]) & (ic[k] < off[k] + shp[k])
        if inb.any():
            total += len(np.unique((ic[2][inb] << 42) | (ic[1][inb] << 21) | ic[0][inb]))
        todo &= ~inb
    return total


STORAGES = ("uint8", "float32")
ROUTINGS = ("default", "rows", "copy")
WARMUP = 20                                   # calls before the timed windows of a case: kernel_times skips as many


def kernel_times(db_path, calls, boxes):
    """Median / 10th / 90th percentile duration (µs) of the timed slice_kernel dispatches of each case, from the rocpd
    database of a traced run of this tool with the same --calls and --boxes."""
    import sqlite3

    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    d = np.array([e - s for n, s, e in rows if "slice_kernel" in n], np.float64) / 1e3
    timed = 2 * boxes * calls
    if len(d) != len(STORAGES) * (1 + len(PLANES) * len(ROUTINGS) * (WARMUP + timed)):
        raise SystemExit(f"{len(d)} slice_kernel dispatches: not a traced run with --calls {calls} --boxes {boxes}")
    i = 0
    for storage in STORAGES:
        i += 1
        for plane, _ in PLANES:
            for routing in ROUTINGS:
                seg = d[i + WARMUP:i + WARMUP + timed]
                i += WARMUP + timed
                print(json.dumps({"storage": storage, "plane": plane, "routing": routing,
                                  "kernel_us": round(float(np.median(seg)), 2),
                                  "kernel_us_p10_p90": [round(float(np.percentile(seg, q)), 2) for q in (10, 90)]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=5)
    ap.add_argument("--volume-n", type=int, default=1024)
    timing.add_interpolation_argument(ap)
    ap.add_argument("--trace-db", default=None, help="attribute the kernels of a traced run instead of timing")
    args = ap.parse_args()
    if args.trace_db:
        return kernel_times(args.trace_db, args.calls, args.boxes)

    import ctypes as C

    import torch

    from sub_volume_renderer_amd import SubVolume, _native as N

    if not torch.cuda.is_available():
        raise SystemExit("slice_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, W, H = args.volume_n, 1920, 1080
    pairs = timing.c2_pairs(n, dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.lib()
    interps = timing.interpolations(args.interpolation)

    for storage in ("native", "float32"):
        spec, scene = timing.c2_scene(n, W, H, "K1", storage, pairs)
        vol = scene.volume
        focus = tuple(float(c) for c in spec.centers[0][0])
        es = {"uint8": 1, "uint16": 2}.get(vol._rings.density_storage, 4)
        print(json.dumps({"storage": vol._rings.density_storage, "frame": [W, H], "volume_n": n, "focus": focus,
                          "blocked_twin": vol._rings.blocked_twin}), flush=True)
        res = vol.render_slice(*SubVolume.axis_slice_plane("z", focus, 1.0), W, H)      # the output tensors
        handle = vol.prepare()
        fb = vol.frame_block(W, H, None)
        ob = N.SliceOutputs.of(res)
        for name, uv in PLANES:
            if uv is None:
                origin, u, v = SubVolume.axis_slice_plane(name, focus, 1.0)
            else:
                origin, (u, v) = focus, uv
            pl = vol._plane_struct(origin, u, v)
            argv = (handle, C.byref(pl), C.byref(fb), C.byref(ob), C.c_void_p(stream.cuda_stream))
            read = texels_read(vol, origin, u, v, W, H) * (es + (4 if vol._rings.labels else 0))

            def one():
                N.check(lib.svr_slice(*argv), "svr_slice")

            for routing, variant, interp in ((r, x, i) for r, x in zip(ROUTINGS, (0, 0x100, 0x200)) for i in interps):
                N.check(lib.svr_set_variant(handle, variant), "svr_set_variant")
                N.check(lib.svr_set_interpolation(handle, N.INTERPOLATIONS[interp]), "svr_set_interpolation")
                call_s, gpu_s = timing.held(one, args.calls, args.boxes, warmup=WARMUP)
                call_us, gpu_us = float(np.median(call_s)) * 1e6, float(np.median(gpu_s)) * 1e6
                written = W * H * (16 + 4 + 4 + 1 + 4 + 1)
                print(json.dumps({"storage": vol._rings.density_storage, "plane": name, "routing": routing, "interpolation": interp,
                                  "call_us": round(call_us, 2), "gpu_us": round(gpu_us, 2),
                                  "call_us_boxes": [round(t * 1e6, 2) for t in call_s],
                                  "gpu_us_boxes": [round(t * 1e6, 2) for t in gpu_s],
                                  "calls_per_box": args.calls, "bytes_written": written,
                                  "write_share_of_6.3TBps_at_gpu_us": round(written / (gpu_us * 1e-6) / HBM_ACHIEVABLE, 3),
                                  "bytes_read_lower_bound": read, "hits": int((res.flags == 2).sum())}), flush=True)
        N.check(lib.svr_set_variant(handle, 0), "svr_set_variant")
        N.check(lib.svr_set_interpolation(handle, 0), "svr_set_interpolation")
        vol.close()
        del vol, res


if __name__ == "__main__":
    main()
