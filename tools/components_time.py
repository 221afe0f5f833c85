#!/usr/bin/env python3
"""Time svr_components (include/svr.h) on a box of up to 512^3 voxels of the finest ring of bench.py's default
configuration (C2: 1024^3, three LODs), on byte rings and on float32 rings: a level set at the median value (one giant
component and specks), a level set at a high level (many small components), and every label split into its pieces, under
6- and 26-connectivity.  HIP events around runs of back-to-back calls on one stream, after a warm-up, the median over
--repeats runs (timing.timed), for the count-only call and for the full call (exact capacities).  One JSON line per
case, beside three references timed in the same run:

1. the count-only svr_mesh call on the same box: one streaming pass over the same ring plus a scan;
2. a device-to-device copy of the ring bytes the call reads;
3. the route a user has today: svr_read_region of the box + scipy.ndimage.label, wall clock (once per case; split by
   label it is scipy on 16 labels of a 64^3 sub-box one by one, scaled by labels and voxels, as the line notes).

usage: python tools/components_time.py [--volume-n 1024] [--box 512] [--repeats 9] [--window 0.2] [--no-cpu]
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
    ap.add_argument("--no-cpu", action="store_true", help="leave the read-back + scipy route out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from sub_volume_renderer_amd import _native as N

    if not torch.cuda.is_available():
        raise SystemExit("components_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.volume_n
    lib = N.lib()
    stream = torch.cuda.current_stream(dev)

    def timed(one):
        return timing.timed(one, args.window, args.repeats, k0=2)          # (the warm-up also allocates the scratch)

    def components_call(vol, box, level, connectivity, ids, records, header):
        cp = N.ComponentsParams(lod=0, use_box=1, connectivity=connectivity)
        cp.box_off[:], cp.box_shape[:] = box
        if level is not None:
            cp.mode, cp.level = N.COMPONENTS_LEVEL, level
        else:
            cp.mode, cp.ignore_zero = N.COMPONENTS_LABELS, 1
        co = N.ComponentsOutputs(None if ids is None else ids.data_ptr(), 0 if ids is None else ids.numel(),
                                 None if records is None else records.data_ptr(), 0 if records is None else records.shape[0], header.data_ptr())
        argv = (vol.prepare(), C.byref(cp), C.byref(co), C.c_void_p(stream.cuda_stream))

        def one():
            N.check(lib.svr_components(*argv), "svr_components")

        one.keep = (cp, co)
        return one

    def mesh_count_seconds(vol, box, level, sel):
        header = torch.empty(8, dtype=torch.int64, device=dev)
        mp = N.MeshParams(lod=0, use_box=1)
        mp.box_off[:], mp.box_shape[:] = box
        if level is not None:
            mp.mode, mp.level = N.MESH_LEVEL, level
        else:
            mp.mode, mp.selected, mp.selected_count = N.MESH_LABELS, sel.data_ptr(), sel.numel()
        mo = N.MeshOutputs(None, None, header.data_ptr(), 0, 0)
        argv = (vol.prepare(), C.byref(mp), C.byref(mo), C.c_void_p(stream.cuda_stream))
        return timed(lambda: N.check(lib.svr_mesh(*argv), "svr_mesh"))[0]

    def cpu_route(vol, box, level, connectivity):
        """svr_read_region of the box + scipy.ndimage.label -> (read seconds, label seconds, components, note)."""
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
        structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
        if level is not None:
            t2 = time.perf_counter()
            count = ndimage.label(den.reshape(shape[::-1]) >= np.float32(level), structure=structure)[1]
            return t1 - t0, time.perf_counter() - t2, count, "whole box"
        e = min(64, *shape)
        sub = lab.reshape(shape[::-1])[:e, :e, :e].copy()
        values = [v for v in np.unique(sub) if v != 0]
        some = values[:16]
        t2 = time.perf_counter()
        count = sum(ndimage.label(sub == v, structure=structure)[1] for v in some)
        per_label = (time.perf_counter() - t2) / max(len(some), 1)
        return (t1 - t0, per_label * len(values) * voxels / float(e ** 3), count,
                f"{len(some)} of the {len(values)} labels of a {e}^3 sub-box one by one, scaled by labels and voxels")

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
        numpy_box = (tuple(box[0][::-1]), tuple(o + s for o, s in zip(box[0][::-1], shape[::-1])))
        # the median value and the 98th percentile as the levels; the label with the most voxels for the mesh reference
        hist = vol.histogram(lod=0, bins=256, range=(0.0, 256.0), box=numpy_box)
        cum = torch.cumsum(hist.counts, 0)
        median = float(int(torch.searchsorted(cum, cum[-1] // 2)) + 1)
        high = float(int(torch.searchsorted(cum, cum[-1] * 98 // 100)) + 1)
        table = vol.objects(lod=0, box=numpy_box)
        sel = table.ids[int(torch.argmax(table.voxels))].reshape(1).to(torch.int32)
        header = torch.empty(16, dtype=torch.int64, device=dev)
        for what, level, connectivity, per_voxel in (("level, median", median, 6, es), ("level, high", high, 6, es), ("level, median", median, 26, es),
                                                     ("every label", None, 6, 4), ("every label", None, 26, 4)):
            count = components_call(vol, box, level, connectivity, None, None, header)
            count_s, c_lo, c_hi, c_k = timed(count)
            head = [int(v) for v in header.cpu().numpy()]
            ids = torch.empty(voxels, dtype=torch.int32, device=dev)
            records = torch.empty((max(head[0], 1), N.COMPONENT_RECORD_BYTES // 4), dtype=torch.int32, device=dev)
            full = components_call(vol, box, level, connectivity, ids, records, header)
            full_s, f_lo, f_hi, f_k = timed(full)
            head = [int(v) for v in header.cpu().numpy()]
            assert head[2] == voxels and head[3] == head[0], head
            largest = int(records.view(torch.int64)[:head[0], 1].max()) if head[0] else 0
            mesh_s = mesh_count_seconds(vol, box, level, sel)
            copy_s = timing.copy_seconds(voxels * per_voxel, args.window, args.repeats, 3)
            line = {
                "case": what, "connectivity": connectivity, "storage": vol._rings.density_storage, "box": shape, "voxels": voxels, "level": level,
                "components": head[0], "inside_voxels": head[1], "largest_component": largest,
                "count_ms": round(count_s * 1e3, 4), "count_ms_min_max": [round(c_lo * 1e3, 4), round(c_hi * 1e3, 4)], "count_calls_per_run": c_k,
                "full_ms": round(full_s * 1e3, 4), "full_ms_min_max": [round(f_lo * 1e3, 4), round(f_hi * 1e3, 4)], "full_calls_per_run": f_k,
                "runs": args.repeats, "ring_bytes_per_voxel": per_voxel,
                "mesh_count_ms": round(mesh_s * 1e3, 4), "count_over_mesh_count": round(count_s / mesh_s, 2),
                "copy_of_ring_bytes_ms": round(copy_s * 1e3, 4), "count_over_copy": round(count_s / copy_s, 2)}
            if not args.no_cpu:
                read_s, label_s, cpu_count, note = cpu_route(vol, box, level, connectivity)
                line.update({"read_region_ms": round(read_s * 1e3, 1), "scipy_label_ms": round(label_s * 1e3, 1), "scipy_components": cpu_count,
                             "scipy_on": note, "today_over_full": round((read_s + label_s) / full_s, 1)})
            print(json.dumps(line), flush=True)
            del ids, records
        vol.close()
        del vol
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
