#!/usr/bin/env python3
"""Time svr_mesh (include/svr.h) on a box of up to 512^3 voxels of the finest ring of bench.py's default configuration
(C2: 1024^3, three LODs): one label, then one level that about half the voxels reach, on byte rings and on float32
rings.  HIP events around runs of back-to-back calls on one stream, after a warm-up, the median over --repeats runs,
for the count-only call and for the emitting call (exact capacities).  One JSON line per case with V, T, the inside
voxels and the ring bytes read per voxel (the element the mode reads, once; SVR_MESH_LEVEL reads the values of an
active cell's corners again: 8 x V elements at the most), beside two references timed in the same run:

1. the route a user has today: svr_read_region of the same box (wall clock) + the numpy restatement tests/mesh_twin.py
   on a 64^3 sub-box, scaled by the number of voxels;
2. svr_objects over the same box, the floor for one streaming pass over the same rings (it reads density AND labels).

usage: python tools/mesh_time.py [--volume-n 1024] [--box 512] [--repeats 9] [--window 0.2]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume-n", type=int, default=1024)
    ap.add_argument("--box", type=int, default=512, help="edge of the box (cut to the window)")
    ap.add_argument("--repeats", type=int, default=9, help="timed runs per case (the median is reported)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed run")
    ap.add_argument("--storages", default="native,float32")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mesh_twin import mesh_twin
    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("mesh_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=3)          # (the warm-up also allocates the scratch)

    def mesh_call(vol, box, sel, level, vertices, triangles, header):
        mp = N.MeshParams(lod=0, use_box=1)
        mp.box_off[:], mp.box_shape[:] = box
        if sel is not None:
            mp.mode, mp.selected, mp.selected_count = N.MESH_LABELS, sel.data_ptr(), sel.numel()
        else:
            mp.mode, mp.level = N.MESH_LEVEL, level
        mo = N.MeshOutputs(None if vertices is None else vertices.data_ptr(), None if triangles is None else triangles.data_ptr(),
                           header.data_ptr(), 0 if vertices is None else vertices.shape[0], 0 if triangles is None else triangles.shape[0])
        argv = (vol.prepare(), C.byref(mp), C.byref(mo), C.c_void_p(stream.cuda_stream))

        def one():
            N.check(lib.svr_mesh(*argv), "svr_mesh")

        one.keep = (mp, mo)
        return one

    def objects_seconds(vol, box):
        records = torch.empty((16384, 12), dtype=torch.int64, device=dev)
        header = torch.empty(8, dtype=torch.int64, device=dev)
        op = N.ObjectsParams(lod=0, capacity=16384, use_box=1)
        op.box_off[:], op.box_shape[:] = box
        oo = N.ObjectsOutputs(records.data_ptr(), header.data_ptr())
        argv = (vol.prepare(), C.byref(op), C.byref(oo), C.c_void_p(stream.cuda_stream))

        return timed(lambda: N.check(lib.svr_objects(*argv), "svr_objects"))[0]

    def readback_route(vol, box, sel_ids, level):
        """svr_read_region of the box (unwrapped pieces of the ring) + the numpy twin on a 64^3 sub-box, scaled."""
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
        e = min(64, *shape)
        den = den.reshape(shape[::-1])[:e, :e, :e].copy()
        lab = lab.reshape(shape[::-1])[:e, :e, :e].copy()
        t2 = time.perf_counter()
        twin = mesh_twin((0, 0, 0), den, lab, selected=sel_ids, level=level)
        t3 = time.perf_counter()
        return (t1 - t0), (t3 - t2) * voxels / float(e ** 3), len(twin["vertices"])

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
        es = {"uint8": 1, "uint16": 2, "float32": 4}[vol._rings.density_storage]
        # the label with the most voxels in the box, and the median value as the level
        table = vol.objects(lod=0, box=(tuple(box[0][::-1]), tuple(o + s for o, s in zip(box[0][::-1], shape[::-1]))))
        label = int(table.ids[int(torch.argmax(table.voxels))])
        hist = vol.histogram(lod=0, bins=256, range=(0.0, 256.0), box=(tuple(box[0][::-1]), tuple(o + s for o, s in zip(box[0][::-1], shape[::-1]))))
        cum = torch.cumsum(hist.counts, 0)
        level = float(int(torch.searchsorted(cum, cum[-1] // 2)) + 1)
        obj_s = objects_seconds(vol, box)
        header = torch.empty(8, dtype=torch.int64, device=dev)
        for what, sel_ids, lvl, per_voxel in (("one label", [label], None, 4), ("one level", None, level, es)):
            sel = None if sel_ids is None else torch.tensor(sel_ids, dtype=torch.int64, device=dev).to(torch.int32)
            count = mesh_call(vol, box, sel, lvl, None, None, header)
            count_s, c_lo, c_hi, c_k = timed(count)
            head = [int(v) for v in header.cpu().numpy()]
            V, T = head[0], head[1]
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
            emit = mesh_call(vol, box, sel, lvl, vertices, triangles, header)
            emit_s, e_lo, e_hi, e_k = timed(emit)
            head = [int(v) for v in header.cpu().numpy()]
            assert head[2] == V and head[3] == T, head
            read_s, twin_s, twin_v = readback_route(vol, box, sel_ids, lvl)
            print(json.dumps({
                "case": what, "storage": vol._rings.density_storage, "box": shape, "voxels": voxels, "label": label if sel_ids else None,
                "level": lvl, "V": V, "T": T, "inside_voxels": head[7],
                "count_ms": round(count_s * 1e3, 4), "count_ms_min_max": [round(c_lo * 1e3, 4), round(c_hi * 1e3, 4)], "count_calls_per_run": c_k,
                "emit_ms": round(emit_s * 1e3, 4), "emit_ms_min_max": [round(e_lo * 1e3, 4), round(e_hi * 1e3, 4)], "emit_calls_per_run": e_k,
                "runs": args.repeats, "ring_bytes_per_voxel": per_voxel, "count_GB_per_s": round(voxels * per_voxel / count_s / 1e9, 1),
                "objects_pass_ms": round(obj_s * 1e3, 4), "count_over_objects_pass": round(count_s / obj_s, 2),
                "read_region_ms": round(read_s * 1e3, 1), "twin_64_cubed_scaled_ms": round(twin_s * 1e3, 1), "twin_64_cubed_vertices": twin_v,
                "today_over_emit": round((read_s + twin_s) / emit_s, 1)}), flush=True)
            del vertices, triangles
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
