#!/usr/bin/env python3
"""Time svr_outline (segmentation outlines, include/svr.h) at 1920 x 1080 on the planes of a BASELINE config 2
render (1024^3, camera K1): HIP events around back-to-back calls on one stream, after a warm-up, over a window of
at least --window seconds, for r in {1, 2, 16} with the depth test off and on.  Per case one JSON line: time per
call, the bytes a call must move (rgba read + written, label, flags, depth when the test is on; no edge mask) and
their share of the HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy reaches).

usage: python tools/outline_time.py [--window 0.5] [--volume-n 1024]
       (for kernel durations without launch gaps: rocprofv3 --kernel-trace --stats -d DIR -- python tools/outline_time.py)
"""
import argparse
import ctypes as C
import json
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--volume-n", type=int, default=1024)
    args = ap.parse_args()

    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("outline_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n, W, H = args.volume_n, 1920, 1080
    scene = timing.c2_scene(n, W, H, "K1")[1]
    res = scene.volume.render(scene.camera, W, H)
    torch.cuda.synchronize()
    hits = int((res.flags == 2).sum())
    out = torch.empty_like(res.rgba)
    colors = torch.from_numpy(scene.volume.material._u["colors"]).to(dev)
    lib, handle = N.lib(), scene.volume._rings.handle
    stream = torch.cuda.current_stream(dev)
    p = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    print(json.dumps({"frame": [W, H], "volume_n": n, "hits": hits}), flush=True)

    for radius in (1, 2, 16):
        for depth_test in (False, True):
            q = N.OutlineParams(radius=radius, depth_tolerance=0.01 if depth_test else -1.0, color_by_label=0,
                                dim_unselected=1.0, only_selected=0)
            q.color[:] = (0.0, 0.0, 0.0, 1.0)
            argv = (handle, p(res.rgba), p(res.depth) if depth_test else None, p(res.label), p(res.flags), W, H,
                    C.byref(q), p(colors), colors.shape[0], None, 0, p(out), None, C.c_void_p(stream.cuda_stream))

            # one window of at least --window seconds, sized from 50 calls after a warm-up of 20
            per_call, _, _, iters = timing.timed(lambda: N.check(lib.svr_outline(*argv), "svr_outline"), args.window,
                                                 repeats=1, k0=50, warmup=20)
            nbytes = W * H * (16 + 16 + 4 + 1 + (4 if depth_test else 0))
            edges = torch.empty((H, W), dtype=torch.uint8, device=dev)
            N.check(lib.svr_outline(*argv[:13], p(edges), argv[14]), "svr_outline")
            torch.cuda.synchronize()
            print(json.dumps({"radius": radius, "depth_test": depth_test, "us_per_call": round(per_call * 1e6, 2),
                              "calls": iters, "window_s": round(per_call * iters, 3), "bytes_per_call": nbytes,
                              "GB_per_s": round(nbytes / per_call / 1e9, 1),
                              "hbm_peak_fraction": round(nbytes / per_call / HBM_PEAK, 3),
                              "edge_pixels": int(edges.sum())}), flush=True)


if __name__ == "__main__":
    main()
