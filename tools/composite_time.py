#!/usr/bin/env python3
"""Time svr_composite (the composite render mode, include/svr.h) at 1920 x 1080 on the BASELINE config 2 scene (1024^3,
the bench's workload) seen from camera K1, for two transfer functions:
  a  faint: alpha <= 0.02 over the whole range, cutoff 1.0 — no ray terminates early, so every ray visits every sample
     (the count is checked against the instrumented march's steps in full LMIP mode, the same rays);
  b  opaque: alpha 0 below 0.3 of the range, rising to 1 at 0.6, cutoff 0.99 — rays stop at the first dense structure.
Called through the C ABI with prebuilt argument structs (steps = NULL: the production call), timed with
the held windows of tools/timing.py:
  call_ms  HIP events around back-to-back calls;
  gpu_ms   the same calls queued behind a sleep kernel (GPU time per call, free of host pacing).
Per case also the samples the kernel visits (the sum of the steps plane of one render with count_steps=True) and
samples per second at gpu_ms.  Kernel durations proper come from a separate traced run, one case per run:

usage: python tools/composite_time.py [--case a|b|all] [--storage native|float32] [--calls 20] [--boxes 3]
       rocprofv3 --kernel-trace --stats --kernel-include-regex composite -d DIR -o comp --output-format csv -- \\
           python tools/composite_time.py --case a --calls 20 --boxes 1
       python tools/composite_time.py --stats DIR          (no GPU needed: the composite kernels of DIR's *kernel_stats.csv)
"""
import argparse
import json
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def transfer_functions():
    from sub_volume_renderer_amd import TransferFunction

    return {
        "a": (TransferFunction.linear(color=(1.0, 0.9, 0.7), opacity=0.02), 1.0),
        "b": (TransferFunction.from_points([(0.0, (0.0, 0.0, 0.0, 0.0)), (0.3, (0.2, 0.3, 0.8, 0.0)),
                                            (0.6, (1.0, 0.7, 0.3, 1.0))]), 0.99),
    }


def stats(path):
    for row in timing.kernel_stats(path, ("composite",), 80):
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=("a", "b", "all"))
    ap.add_argument("--storage", default="native", choices=("native", "float32"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=3)
    ap.add_argument("--volume-n", type=int, default=1024)
    timing.add_interpolation_argument(ap)
    ap.add_argument("--cut", default="none", choices=("none", "half", "wedge", "all-cases"),
                    help="svr_set_cut_planes state of the timed calls (tools/cut_cases.py: planes through the camera's focus "
                         "that open the side towards the camera); all-cases: none, half and wedge alternate, case by case")
    ap.add_argument("--stats", default=None, help="print the composite kernels of a --stats run's CSV instead of timing")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)

    import ctypes as C

    import torch

    import cut_cases
    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("composite_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n_vol, W, H = args.volume_n, 1920, 1080
    stream = torch.cuda.current_stream(dev)
    lib = N.lib()
    spec, scene = timing.c2_scene(n_vol, W, H, "K1", args.storage)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    print(json.dumps({"storage": vol._rings.density_storage, "frame": [W, H], "volume_n": n_vol, "camera": "K1"}), flush=True)
    lmip_full = None
    for case, (tf, cutoff) in transfer_functions().items():
        if args.case not in ("all", case):
            continue
        if case == "a":
            # the instrumented march in full LMIP mode (threshold +inf: no sample is significant) visits every sample
            m.render_mode, threshold = "lmip", m.lmip_threshold
            m.lmip_threshold = float("inf")
            lmip_full = int(vol.render(cam, W, H, count_steps=True).steps.to(torch.int64).sum())
            m.lmip_threshold = threshold
        m.render_mode, m.transfer_function, m.alpha_cutoff, m.color_by_label = "composite", tf, cutoff, False
        for cut in cut_cases.names_of(args.cut):
            planes, mode = cut_cases.cut_case(cut, spec.cam_position, spec.cam_target)
            m.cut_planes, m.cut_mode = planes, mode
            res = vol.render(cam, W, H, count_steps=True)
            samples = int(res.steps.to(torch.int64).sum())
            hits = int((res.flags == N.SVR_PIX_HIT).sum())
            handle = vol.prepare()
            vol._push_transfer_function()
            cb, fb = vol.camera_block(cam), vol.frame_block(W, H, None)
            cp = N.CompositeParams(cutoff, 0)
            ob = N.Outputs.of(res, pick_id=vol.id)
            argv = (handle, C.byref(cb), C.byref(fb), C.byref(cp), C.byref(ob), C.c_void_p(stream.cuda_stream))

            def one():
                N.check(lib.svr_composite(*argv), "svr_composite")

            for interp in timing.interpolations(args.interpolation):
                # (samples and hit_pixels are the nearest render's: the rays are the same, linear values end some earlier or later)
                N.check(lib.svr_set_interpolation(handle, N.INTERPOLATIONS[interp]), "svr_set_interpolation")
                N.check(cut_cases.push(lib, handle, planes, mode, N.CUT_MODES), "svr_set_cut_planes")
                call_s, gpu_s = timing.held(one, args.calls, args.boxes, warmup=5)
                gpu = float(np.median(gpu_s))
                row = {"case": case, "storage": vol._rings.density_storage, "interpolation": interp, "cut": cut, "table_entries": tf.size,
                       "alpha_cutoff": cutoff, "call_ms": round(float(np.median(call_s)) * 1e3, 4), "gpu_ms": round(gpu * 1e3, 4),
                       "gpu_ms_boxes": [round(t * 1e3, 4) for t in gpu_s],
                       "calls_per_box": args.calls, "samples": samples, "samples_per_s": float(f"{samples / gpu:.4g}"),
                       "hit_pixels": hits}
                if case == "a":
                    row["lmip_full_samples"] = lmip_full
                print(json.dumps(row), flush=True)
        m.cut_planes = ()
        N.check(lib.svr_set_interpolation(handle, 0), "svr_set_interpolation")
        N.check(cut_cases.push(lib, handle, [], "ANY", N.CUT_MODES), "svr_set_cut_planes")
    vol.close()


if __name__ == "__main__":
    main()
