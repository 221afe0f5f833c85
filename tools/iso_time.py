#!/usr/bin/env python3
"""Time svr_iso (the iso-surface render mode, include/svr.h) at 1920 x 1080 on the BASELINE config 2 scene (1024^3, the
bench's workload) from camera K1 or the inside camera K2, against its two yardsticks on the same box in the same run:
  iso        svr_iso with empty-space skipping (the default);
  iso_noskip svr_iso with no_skip = 1 (every stretch marched);
  A          svr_composite with a step table (alpha 0 below the level, 1 at and above it), alpha_cutoff 0.99: the same
             rays, stopped at the same coarse sample, no skipping;
  B          the LMIP march (svr_render) at lmip_threshold = iso_value: the bench's workload.
Called through the C ABI with prebuilt argument structs (steps = NULL: the production calls), timed with
the held windows of tools/timing.py:
  call_ms  HIP events around back-to-back calls;
  gpu_ms   the same calls queued behind a sleep kernel (GPU time per call, free of host pacing), the median of
           --boxes windows, with their min and max (the run-to-run spread).
The four are timed in alternation, --rounds times.  Also printed: the hit pixels, the coarse samples the definition
visits (the steps plane), and the wave-stretches marched and skipped (svr_iso_params::skip_counters).  Kernel durations
proper come from a separate traced run:

--cut none|half|wedge|all-cases: the svr_set_cut_planes state of the timed svr_iso and svr_composite calls (tools/
cut_cases.py: planes through the camera's focus that open the side towards the camera); all-cases: the three alternate
case by case inside one command and every row names its cut.  The march (B) knows no cuts and runs under "none" only.

usage: python tools/iso_time.py [--camera K1|K2] [--storage native|float32] [--level 0.5] [--calls 20] [--boxes 3]
       rocprofv3 --kernel-trace --stats -d DIR -o iso --output-format csv -- python tools/iso_time.py --calls 20 --boxes 1
       python tools/iso_time.py --stats DIR          (no GPU needed: the kernels of DIR's *kernel_stats.csv)
"""
import argparse
import json
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _NoExtraPlanes:
    normal = None
    skip_counters = None


def stats(path):
    for row in timing.kernel_stats(path, ("iso_kernel", "composite_kernel", "march_"), 90):
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--camera", default="K1", choices=("K1", "K2"))
    ap.add_argument("--storage", default="native", choices=("native", "float32"))
    ap.add_argument("--level", type=float, default=0.5, help="iso_value as a fraction of the data range (the bench's LMIP threshold: 0.5)")
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--only", default=None, help="comma-separated subset of iso,iso_noskip,A,B (a traced or counted run of one kernel)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--volume-n", type=int, default=1024)
    timing.add_interpolation_argument(ap)
    ap.add_argument("--cut", default="none", choices=("none", "half", "wedge", "all-cases"),
                    help="cut planes of the timed iso / composite calls; all-cases: none, half and wedge alternate")
    ap.add_argument("--stats", default=None, help="print the kernels of a --stats run's CSV instead of timing")
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)

    import ctypes as C

    import torch

    import cut_cases
    from sub_volume_renderer_amd import TransferFunction, _native as N

    if not torch.cuda.is_available():
        raise SystemExit("iso_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n_vol, W, H = args.volume_n, 1920, 1080
    stream = torch.cuda.current_stream(dev)
    lib = N.lib()
    spec, scene = timing.c2_scene(n_vol, W, H, args.camera, args.storage)
    vol, cam = scene.volume, scene.camera
    m = vol.material
    level = args.level * 255.0
    m.lmip_threshold = level
    m.iso_value, m.iso_refine = level, args.refine
    # yardstick A's table over clim = (0, 255): entry k is the value k; alpha steps from 0 to 1 at the level
    table = np.zeros((256, 4), np.float32)
    table[:, :3] = 0.8
    table[int(np.ceil(level)):, 3] = 1.0
    m.transfer_function, m.alpha_cutoff, m.color_by_label = TransferFunction(table), 0.99, False
    print(json.dumps({"storage": vol._rings.density_storage, "frame": [W, H], "volume_n": n_vol, "camera": args.camera,
                      "iso_value": level, "refine": args.refine}), flush=True)

    interps = timing.interpolations(args.interpolation)
    cuts = {c: cut_cases.cut_case(c, spec.cam_position, spec.cam_target) for c in cut_cases.names_of(args.cut)}
    # one counted render of each (steps planes, skip counters), then the production argument structs
    m.render_mode = "iso"
    info = {}
    for cut in [c for c in cuts if c != "none"] + ["none"]:
        m.cut_planes, m.cut_mode = cuts.get(cut, ([], "ANY"))
        for interp in [i for i in interps if i != "nearest"] + ["nearest"]:     # (nearest, uncut last: what the yardsticks below compare with)
            m.interpolation = interp
            out = vol.iso_outputs(W, H, count_steps=True, normal=False, skip_counters=True)
            vol.render(cam, W, H, count_steps=True, out=out)
            torch.cuda.synchronize()
            marched, skipped = (int(v) for v in out.skip_counters.cpu().numpy().view(np.uint32))
            info[("iso", interp, cut)] = {"hit_pixels": int((out.flags == N.SVR_PIX_HIT).sum()),
                                          "coarse_samples": int(out.steps.to(torch.int64).sum()),
                                          "wave_stretches_marched": marched, "wave_stretches_skipped": skipped,
                                          "skipped_share": round(skipped / max(marched + skipped, 1), 4)}
    iso_steps = out.steps.clone()
    m.render_mode = "composite"
    res = vol.render(cam, W, H, count_steps=True)
    torch.cuda.synchronize()
    info[("A", "nearest", "none")] = {"hit_pixels": int((res.flags == N.SVR_PIX_HIT).sum()), "samples": int(res.steps.to(torch.int64).sum()),
                 "pixels_with_iso_steps": int((res.steps == iso_steps).sum())}
    m.render_mode = "lmip"
    res = vol.render(cam, W, H)
    torch.cuda.synchronize()
    info[("B", "nearest", "none")] = {"hit_pixels": int((res.flags == N.SVR_PIX_HIT).sum())}

    handle = vol.prepare()
    vol._push_transfer_function()
    cb, fb = vol.camera_block(cam), vol.frame_block(W, H, None)
    ob = N.Outputs.of(res, pick_id=vol.id)
    ip_on = vol._iso_params(_NoExtraPlanes)
    ip_off = vol._iso_params(_NoExtraPlanes)
    ip_off.no_skip = 1
    cp = N.CompositeParams(0.99, 0)
    s = C.c_void_p(stream.cuda_stream)
    runs = {
        "iso": lambda: N.check(lib.svr_iso(handle, C.byref(cb), C.byref(fb), C.byref(ip_on), C.byref(ob), s), "svr_iso"),
        "iso_noskip": lambda: N.check(lib.svr_iso(handle, C.byref(cb), C.byref(fb), C.byref(ip_off), C.byref(ob), s), "svr_iso"),
        "A": lambda: N.check(lib.svr_composite(handle, C.byref(cb), C.byref(fb), C.byref(cp), C.byref(ob), s), "svr_composite"),
        "B": lambda: N.check(lib.svr_render(handle, C.byref(cb), C.byref(fb), C.byref(ob), s), "svr_render"),
    }
    if args.only:
        runs = {k: v for k, v in runs.items() if k in args.only.split(",")}
    for rnd in range(args.rounds):
        for name, one, interp, cut in ((n, o, i, c) for n, o in runs.items() for i in (interps if n != "B" else ("nearest",))
                                       for c in (cuts if n != "B" else ("none",))):
            N.check(lib.svr_set_interpolation(handle, N.INTERPOLATIONS[interp]), "svr_set_interpolation")
            N.check(cut_cases.push(lib, handle, *cuts.get(cut, ([], "ANY")), N.CUT_MODES), "svr_set_cut_planes")
            call_s, gpu_s = timing.held(one, args.calls, args.boxes, warmup=5)
            row = {"case": name, "interpolation": interp, "cut": cut, "round": rnd, "call_ms": round(float(np.median(call_s)) * 1e3, 4),
                   "gpu_ms": round(float(np.median(gpu_s)) * 1e3, 4), "gpu_ms_min": round(min(gpu_s) * 1e3, 4),
                   "gpu_ms_max": round(max(gpu_s) * 1e3, 4), "calls_per_box": args.calls}
            row.update(info.get(("iso" if name.startswith("iso") else name, interp, cut), {}))
            print(json.dumps(row), flush=True)
    N.check(lib.svr_set_interpolation(handle, 0), "svr_set_interpolation")
    N.check(cut_cases.push(lib, handle, [], "ANY", N.CUT_MODES), "svr_set_cut_planes")
    vol.close()


if __name__ == "__main__":
    main()
