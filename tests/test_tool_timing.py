"""tools/timing.py (what the tools/*_time.py scripts share) and the two output-struct builders of _native, without a
GPU: the pure halves of the two timing methods, the reader of a traced run's kernel statistics, `Outputs.of` /
`SliceOutputs.of` against the field-by-field fills they replaced, and the scripts' command lines (the --stats /
--trace-db paths must not import torch)."""
import itertools
import json
import os
import sqlite3
import subprocess
import sys
from types import SimpleNamespace

import pytest

from sub_volume_renderer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

import timing  # noqa: E402

TIME_SCRIPTS = ("slice_time", "slab_time", "composite_time", "iso_time", "histogram_time", "objects_time", "mesh_time",
                "outline_time")


# ---- the pure halves of the two methods ------------------------------------------------
def test_hold_cycles_is_four_times_the_slowest_window_and_at_least_20_ms():
    assert timing.hold_cycles([1e-3, 2e-3], 10, 1e-9) == int(0.08 / 1e-9)             # 4 x 2 ms x 10 calls
    assert timing.hold_cycles([1e-6, 2e-6], 10, 1e-9) == int(0.02 / 1e-9)             # 4 x 20 us < 20 ms
    assert timing.hold_cycles([4e-4, 5e-4], 10, 2.5e-9) == int(0.02 / 2.5e-9)         # exactly 20 ms either way
    assert timing.hold_cycles([3e-3], 7, 4e-10) == int(4.0 * 3e-3 * 7 / 4e-10)


def test_calls_for_window():
    assert timing.calls_for_window(0.5, 0.2, 10) == 10                                # one call fills the window: the floor
    assert timing.calls_for_window(0.2, 0.2, 5) == 5
    assert timing.calls_for_window(1e-4, 0.2, 10) == int(0.2 / 1e-4) + 1
    assert timing.calls_for_window(3e-6, 0.5, 50) == int(0.5 / 3e-6) + 1
    assert timing.calls_for_window(0.0, 0.02, 3) == int(0.02 / 1e-7) + 1              # no division by zero
    assert timing.calls_for_window(2e-3, 0.02, 3) == 11                               # above the floor by a few calls


# ---- the --stats reader ---------------------------------------------------------------
COMPOSITE_NAME = ("void composite_kernel<unsigned char, 3, true, false>(svr_device_context const*, svr_camera, svr_frame, "
                  "svr_composite_params, svr_outputs) [clone .kd]")
ISO_NAME = "void iso_kernel<float, 3, false>(svr_device_context const*, svr_camera, svr_frame, svr_iso_params) [clone .kd]"
SLICE_NAME = "slice_kernel(svr_device_context const*, svr_slice_plane, svr_frame, svr_slice_outputs)"
# what the stats() of composite_time.py and of iso_time.py printed for the file below before they shared a reader
COMPOSITE_ROWS = [
    {"file": "x_kernel_stats.csv", "kernel": "void composite_kernel<unsigned char, 3, true, false>(svr_device_context const*, ",
     "calls": 25, "average_ms": 1.8346, "min_ms": 1.79, "max_ms": 1.9012},
]
ISO_ROWS = [
    {"file": "x_kernel_stats.csv", "kernel": "void composite_kernel<unsigned char, 3, true, false>(svr_device_context const*, svr_camera",
     "calls": 25, "average_ms": 1.8346, "min_ms": 1.79, "max_ms": 1.9012},
    {"file": "x_kernel_stats.csv", "kernel": "void iso_kernel<float, 3, false>(svr_device_context const*, svr_camera, svr_frame, svr_iso",
     "calls": 45, "average_ms": 0.9123, "min_ms": 0.9, "max_ms": 0.935},
]


@pytest.fixture()
def stats_dir(tmp_path):
    with open(tmp_path / "x_kernel_stats.csv", "w") as f:
        f.write('"Name","Calls","AverageNs","MinNs","MaxNs"\n')
        f.write(f'"{COMPOSITE_NAME}",25,1834567.25,1790012,1901234\n')
        f.write(f'"{ISO_NAME}",45,912345.5,900001,934999\n')
        f.write(f'"{SLICE_NAME}",7,25123.4,24000,27000\n')
    return str(tmp_path)


def test_kernel_stats_filters_and_widths(stats_dir):
    assert len(COMPOSITE_NAME) > 90 and len(ISO_NAME) > 90
    composite = timing.kernel_stats(stats_dir, ("composite",), 80)
    iso = timing.kernel_stats(stats_dir, ("iso_kernel", "composite_kernel", "march_"), 90)
    assert composite == COMPOSITE_ROWS and [list(r) for r in composite] == [list(r) for r in COMPOSITE_ROWS]
    assert iso == ISO_ROWS and [list(r) for r in iso] == [list(r) for r in ISO_ROWS]
    assert len(composite[0]["kernel"]) == 80 and all(len(r["kernel"]) == 90 for r in iso)
    assert timing.kernel_stats(stats_dir, ("march_",), 90) == []


# ---- the two output-struct builders ---------------------------------------------------------
class Plane:
    """Stands in for a device tensor: all the builders ask of it is its address."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def _fields(struct):
    return {name: getattr(struct, name) for name, _ in struct._fields_}


def _outputs_as_render_filled_them(res, count_steps, pick, vol_id):
    """The block of SubVolume.render that `Outputs.of` replaced, field by field."""
    ob = N.Outputs()
    ob.rgba = res.rgba.data_ptr()
    ob.depth = res.depth.data_ptr() if res.depth is not None else None
    ob.label = res.label.data_ptr() if res.label is not None else None
    ob.flags = res.flags.data_ptr() if res.flags is not None else None
    ob.steps = res.steps.data_ptr() if (count_steps and res.steps is not None) else None
    ob.pick = res.pick.data_ptr() if (pick and res.pick is not None) else None
    ob.pick_id = vol_id & 0xFFFFFFFF
    return ob


def _slice_outputs_as_plane_ob_filled_them(res):
    """SubVolume._plane_ob before it called `SliceOutputs.of`."""
    ob = N.SliceOutputs()
    for name in ("rgba", "depth", "label", "flags", "value", "lod"):
        t = getattr(res, name)
        setattr(ob, name, t.data_ptr() if t is not None else None)
    return ob


def test_outputs_of_matches_the_fill_of_render():
    cases = 0
    for have_steps, have_pick, want_steps, want_pick, have_depth, have_label, have_flags in itertools.product((False, True), repeat=7):
        res = SimpleNamespace(rgba=Plane(0x1000), depth=Plane(0x2000) if have_depth else None,
                              label=Plane(0x3000) if have_label else None, flags=Plane(0x4000) if have_flags else None,
                              steps=Plane(0x5000) if have_steps else None, pick=Plane(0x6000) if have_pick else None)
        for vol_id in (0, 7, 0x1_2345_6789):
            got = N.Outputs.of(res, steps=want_steps, pick=want_pick, pick_id=vol_id & 0xFFFFFFFF)
            want = _outputs_as_render_filled_them(res, want_steps, want_pick, vol_id)
            assert _fields(got) == _fields(want), (have_steps, have_pick, want_steps, want_pick, vol_id)
            assert bytes(got) == bytes(want)
            cases += 1
    assert cases == 128 * 3
    # spelled out once: asked for and present, asked for and absent, present and not asked for
    res = SimpleNamespace(rgba=Plane(16), depth=Plane(32), label=None, flags=Plane(64), steps=Plane(128), pick=None)
    assert _fields(N.Outputs.of(res, steps=True, pick=True, pick_id=9)) == {
        "rgba": 16, "depth": 32, "label": None, "flags": 64, "steps": 128, "pick": None, "pick_id": 9}
    assert _fields(N.Outputs.of(res)) == {
        "rgba": 16, "depth": 32, "label": None, "flags": 64, "steps": None, "pick": None, "pick_id": 0}


def test_slice_outputs_of_matches_plane_ob():
    names = ("depth", "label", "flags", "value", "lod")
    for have in itertools.product((False, True), repeat=len(names)):
        res = SimpleNamespace(rgba=Plane(0x100), steps=None, pick=None,
                              **{n: Plane(0x200 * (k + 2)) if h else None for k, (n, h) in enumerate(zip(names, have))})
        got, want = N.SliceOutputs.of(res), _slice_outputs_as_plane_ob_filled_them(res)
        assert _fields(got) == _fields(want) and bytes(got) == bytes(want), have
    assert _fields(N.SliceOutputs.of(res)) == {"rgba": 0x100, "depth": 0x400, "label": 0x600, "flags": 0x800, "value": 0xA00,
                                               "lod": 0xC00}
    from sub_volume_renderer_amd import SubVolume

    assert bytes(SubVolume._plane_ob(res)) == bytes(want)


# ---- the scripts' command lines ----------------------------------------------------------------
@pytest.mark.parametrize("script", TIME_SCRIPTS)
def test_time_script_parses(script):
    run = subprocess.run([sys.executable, os.path.join(TOOLS, script + ".py"), "--help"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.startswith("usage: " + script + ".py")


def _run_without_torch(script, *args):
    """The script as `python tools/<script>.py args`, in a process where `import torch` raises."""
    path = os.path.join(TOOLS, script + ".py")
    code = ("import runpy, sys; sys.modules['torch'] = None; "
            f"sys.path.insert(0, {TOOLS!r}); sys.argv = [{path!r}, *{list(args)!r}]; "
            f"runpy.run_path({path!r}, run_name='__main__')")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return [json.loads(line) for line in run.stdout.splitlines()]


def test_stats_paths_need_no_torch(stats_dir):
    assert _run_without_torch("composite_time", "--stats", stats_dir) == COMPOSITE_ROWS
    assert _run_without_torch("iso_time", "--stats", stats_dir) == ISO_ROWS


def test_trace_db_paths_need_no_torch_and_count_the_calls_held_issues(tmp_path):
    """--trace-db accepts exactly the dispatches a run issues: per ring type the allocating calls, then per case the
    script's warm-up + 2 x boxes x calls (what timing.held invokes), and prints one row per case."""
    import slab_time
    import slice_time

    calls, boxes = 3, 2
    per_case = slice_time.WARMUP + 2 * boxes * calls
    assert slice_time.WARMUP == 20 and slab_time.WARMUP == 20

    def database(name, kernels):
        db = sqlite3.connect(tmp_path / name)
        db.execute("create table kernels (name text, start integer, end integer)")
        db.executemany("insert into kernels values (?, ?, ?)", [(k, 1000 * i, 1000 * i + 500 + i % 7) for i, k in enumerate(kernels)])
        db.commit()
        db.close()
        return str(tmp_path / name)

    slice_cases = len(slice_time.PLANES) * len(slice_time.ROUTINGS)
    one_storage = ["slice_kernel<0>"] * (1 + slice_cases * per_case)
    rows = _run_without_torch("slice_time", "--calls", str(calls), "--boxes", str(boxes), "--trace-db",
                              database("slice.db", ["fill_kernel"] + one_storage * 2))
    assert len(rows) == 2 * slice_cases
    assert [r["storage"] for r in rows] == ["uint8"] * slice_cases + ["float32"] * slice_cases
    assert list(rows[0]) == ["storage", "plane", "routing", "kernel_us", "kernel_us_p10_p90"]

    slab_cases = list(slab_time.cases())
    one_storage = ["slice_kernel<0>", "slab_kernel<0>"]
    for kind, *_ in slab_cases:
        one_storage += [kind + "_kernel<0>"] * per_case
    rows = _run_without_torch("slab_time", "--calls", str(calls), "--boxes", str(boxes), "--trace-db",
                              database("slab.db", one_storage * 2))
    assert len(rows) == 2 * len(slab_cases)
    assert list(rows[0]) == ["storage", "kind", "slab", "samples", "mode", "routing", "kernel_us", "kernel_us_p10_p90"]
    # one dispatch short: not this run
    path = os.path.join(TOOLS, "slice_time.py")
    short = subprocess.run([sys.executable, path, "--calls", str(calls), "--boxes", str(boxes), "--trace-db",
                            database("short.db", (["slice_kernel<0>"] * (1 + slice_cases * per_case) * 2)[:-1])],
                           capture_output=True, text=True)
    assert short.returncode != 0 and "not a traced run" in short.stderr
