#!/usr/bin/env python3
"""Time svr_slab (thick-slab projections, include/svr.h) at 1920 x 1080 on the BASELINE config 2 scene (1024^3, the
bench's workload) with byte rings and with float32 rings: z-, x-normal and one oblique slab through the camera's focus
at 1 voxel per pixel and 1 voxel per sample, N in {1, 16, 64}, max and mean, with the default routing of the
micro-block copy, rows only (variant bit 8) and the copy always (bit 9); plus svr_slice on the z-normal plane, the
N = 1 yardstick.  Called through the C ABI with prebuilt argument structs, timed with the held windows of tools/timing.py:
  call_us  HIP events around back-to-back calls;
  gpu_us   the same calls queued behind a sleep kernel (GPU time per call, free of host pacing).
Per case also the two floors:
  bytes_floor_us  (bytes written + distinct texels read, each element once) / 6.3 TB/s;
  valu_floor_us   samples inside the box x VALU per sample (--valu-per-sample, counted in the ISA of slab_kernel's
                  loop) / 64 lanes x the measured issue time of a VALU wave-instruction (1.06 ns per SIMD at 8 waves,
                  profiles/r01/ubench_valu_issue_rate.txt) / 1024 SIMDs.
Kernel durations proper come from a separate traced run, whose dispatches --trace-db attributes to the cases by order
(per ring type: one slice and one slab dispatch that allocate the outputs, then per case 20 warm-up + 2 x boxes x calls):

usage: python tools/slab_time.py [--calls 50] [--boxes 3]
       rocprofv3 --kernel-trace -d DIR -o slab -- python tools/slab_time.py --calls 20 --boxes 2
       python tools/slab_time.py --calls 20 --boxes 2 --trace-db DIR/slab_results.db     (no GPU needed)
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
VALU_NS_PER_WAVE_INSTR = 1.06          # v_add_f32 at 8 waves / SIMD, profiles/r01/ubench_valu_issue_rate.txt
SIMDS = 256 * 4
STORAGES = ("uint8", "float32")
SLABS = ("z", "x", "oblique")
SAMPLES = (1, 16, 64)
MODES = ("max", "mean")
ROUTINGS = ("default", "rows", "copy")
OBLIQUE = ((0.8, 0.6, 0.0), (-0.36, 0.48, 0.8), (0.48, -0.64, 0.6))     # u, v, w: orthonormal
WARMUP = 20                                   # calls before the timed windows of a case: kernel_times skips as many


def cases():
    yield ("slice", "z", 1, "max", "default")
    for s in SLABS:
        for n in SAMPLES:
            for mode in MODES:
                for routing in ROUTINGS:
                    yield ("slab", s, n, mode, routing)


def kernel_times(db_path, calls, boxes):
    import sqlite3

    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    d = [(("slab" if "slab_kernel" in n else "slice"), (e - s) / 1e3) for n, s, e in rows
         if "slab_kernel" in n or "slice_kernel" in n]
    timed = 2 * boxes * calls
    per = list(cases())
    if len(d) != len(STORAGES) * (2 + len(per) * (WARMUP + timed)):
        raise SystemExit(f"{len(d)} slice / slab dispatches: not a traced run with --calls {calls} --boxes {boxes}")
    i = 0
    for storage in STORAGES:
        i += 2
        for kind, s, n, mode, routing in per:
            seg = np.array([t for k, t in d[i + WARMUP:i + WARMUP + timed]])
            assert all(k == kind for k, _ in d[i:i + WARMUP + timed])
            i += WARMUP + timed
            print(json.dumps({"storage": storage, "kind": kind, "slab": s, "samples": n, "mode": mode, "routing": routing,
                              "kernel_us": round(float(np.median(seg)), 2),
                              "kernel_us_p10_p90": [round(float(np.percentile(seg, q)), 2) for q in (10, 90)]}))


def footprint(vol, origin, u, v, w, n, W, H):
    """(samples inside the box, distinct (LOD, voxel) texels the slab reads), from the definition in svr.h evaluated
    with torch float32 on the GPU (a measurement aid: float details do not matter to a count)."""
    import torch

    dev = torch.device("cuda", 0)
    f = torch.float32
    size = torch.tensor(np.asarray(vol._volume_dimensions, np.float32), device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=f), torch.arange(W, device=dev, dtype=f), indexing="ij")
    fx, fy = (xs + 0.5) - 0.5 * W, (ys + 0.5) - 0.5 * H
    m = torch.tensor(np.asarray(vol.world.inverse_matrix, np.float32), device=dev)
    p = [(origin[k] + fx * u[k]) + fy * v[k] for k in range(3)]
    q = [((m[k, 0] * p[0] + m[k, 1] * p[1]) + m[k, 2] * p[2]) + m[k, 3] for k in range(3)]
    dw = [float((m[k, 0] * w[0] + m[k, 1] * w[1]) + m[k, 2] * w[2]) for k in range(3)]
    inside_total, keys = 0, []
    for k in range(n):
        t = k - 0.5 * (n - 1)
        d = [(q[i] + t * dw[i]) + 0.5 for i in range(3)]
        todo = (d[0] >= 0) & (d[0] < size[0]) & (d[1] >= 0) & (d[1] < size[1]) & (d[2] >= 0) & (d[2] < size[2])
        inside_total += int(todo.sum())
        for l, b in enumerate(vol.wrapping_buffers):
            st = b.uniform_buffer.data
            off, shp = st["current_logical_offset_in_pixels"], st["current_logical_shape_in_pixels"]
            scale = b.scale_factor[::-1]
            ic = [torch.where(todo, d[i] * float(scale[i]), 0).to(torch.int64) for i in range(3)]
            inb = todo.clone()
            for i in range(3):
                inb &= (int(off[i]) <= ic[i]) & (ic[i] < int(off[i]) + int(shp[i]))
            keys.append(((l << 60) | (ic[2][inb] << 40) | (ic[1][inb] << 20) | ic[0][inb]).unique())
            todo &= ~inb
    return inside_total, int(torch.cat(keys).unique().numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--boxes", type=int, default=3)
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--valu-per-sample", type=float, default=None,
                    help="VALU per sample of slab_kernel's loop, from its ISA (DESIGN.md); omit: no VALU floor")
    timing.add_interpolation_argument(ap)
    ap.add_argument("--trace-db", default=None, help="attribute the kernels of a traced run instead of timing")
    args = ap.parse_args()
    if args.trace_db:
        return kernel_times(args.trace_db, args.calls, args.boxes)

    import ctypes as C

    import torch

    from sub_volume_renderer_amd import SubVolume, _native as N

    if not torch.cuda.is_available():
        raise SystemExit("slab_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n_vol, W, H = args.volume_n, 1920, 1080
    pairs = timing.c2_pairs(n_vol, dev)
    stream = torch.cuda.current_stream(dev)
    lib = N.lib()
    interps = timing.interpolations(args.interpolation)
    written = W * H * (16 + 4 + 4 + 1 + 4 + 1)

    for storage in ("native", "float32"):
        spec, scene = timing.c2_scene(n_vol, W, H, "K1", storage, pairs)
        vol = scene.volume
        focus = tuple(float(c) for c in spec.centers[0][0])
        es = {"uint8": 1, "uint16": 2}.get(vol._rings.density_storage, 4)
        print(json.dumps({"storage": vol._rings.density_storage, "frame": [W, H], "volume_n": n_vol, "focus": focus,
                          "blocked_twin": vol._rings.blocked_twin}), flush=True)
        o, u, v = SubVolume.axis_slice_plane("z", focus, 1.0)
        res_slice = vol.render_slice(o, u, v, W, H)                       # the output tensors
        res = vol.render_slab(o, u, v, (0.0, 0.0, 1.0), 1, W, H)
        handle = vol.prepare()
        fb = vol.frame_block(W, H, None)
        ob_slice, ob_slab = N.SliceOutputs.of(res_slice), N.SliceOutputs.of(res)
        foot = {}
        for kind, s, n, mode, routing, interp in ((*c, i) for c in cases() for i in interps):
            if s == "oblique":
                origin, (u, v, w) = focus, OBLIQUE
            else:
                origin, u, v, w = SubVolume.axis_slab_plane(s, focus, 1.0, 1.0)
            pl = vol._plane_struct(origin, u, v)
            if kind == "slice":
                argv = (handle, C.byref(pl), C.byref(fb), C.byref(ob_slice), C.c_void_p(stream.cuda_stream))
                fn, name = lib.svr_slice, "svr_slice"
            else:
                sp = N.SlabParams()
                sp.plane = pl
                sp.w[:] = w
                sp.w_len, sp.samples, sp.mode = float(np.linalg.norm(w)), n, N.SLAB_MODES[mode]
                argv = (handle, C.byref(sp), C.byref(fb), C.byref(ob_slab), C.c_void_p(stream.cuda_stream))
                fn, name = lib.svr_slab, "svr_slab"
            if (s, n) not in foot:
                foot[(s, n)] = footprint(vol, origin, u, v, w, n, W, H)
            inside, texels = foot[(s, n)]

            def one():
                N.check(fn(*argv), name)

            N.check(lib.svr_set_variant(handle, {"default": 0, "rows": 0x100, "copy": 0x200}[routing]), "svr_set_variant")
            N.check(lib.svr_set_interpolation(handle, N.INTERPOLATIONS[interp]), "svr_set_interpolation")
            call_s, gpu_s = timing.held(one, args.calls, args.boxes, warmup=WARMUP)
            read = texels * (es + (4 if vol._rings.labels else 0))
            row = {"storage": vol._rings.density_storage, "kind": kind, "slab": s, "samples": n, "mode": mode,
                   "routing": routing, "interpolation": interp, "call_us": round(float(np.median(call_s)) * 1e6, 2),
                   "gpu_us": round(float(np.median(gpu_s)) * 1e6, 2), "calls_per_box": args.calls,
                   "samples_inside": inside, "bytes_written": written, "bytes_read_floor": read,
                   "bytes_floor_us": round((written + read) / HBM_ACHIEVABLE * 1e6, 2)}
            if args.valu_per_sample and kind == "slab":
                row["valu_floor_us"] = round(inside / 64 * args.valu_per_sample * VALU_NS_PER_WAVE_INSTR / SIMDS / 1e3, 2)
            print(json.dumps(row), flush=True)
        N.check(lib.svr_set_variant(handle, 0), "svr_set_variant")
        N.check(lib.svr_set_interpolation(handle, 0), "svr_set_interpolation")
        vol.close()
        del vol, res, res_slice


if __name__ == "__main__":
    main()
