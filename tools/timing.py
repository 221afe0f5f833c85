"""What the tools/*_time.py scripts share: the two ways a call is timed, the memcpy yardstick, the reader of a traced
run's kernel statistics and the BASELINE config 2 scene they all measure on.  A plain module beside the scripts
(``import timing``), not part of the package; torch is imported inside the functions that need a GPU, so the
--stats / --trace-db paths of the scripts run without one.

The held-window method (``held``): what slices, slabs, composites and iso renders are timed with.  Per case a warm-up,
then --boxes windows of --calls back-to-back calls between two HIP events (call_s: host enqueue and device both count),
then the same windows enqueued while a sleep kernel holds the stream, the events recorded behind it (gpu_s: the device
drains a full queue, so kernel + dispatch gap, free of host pacing).

The fill-a-window method (``timed``): what the histogram, objects, mesh and outline passes are timed with.  A warm-up,
k0 calls timed to size a run of k calls to --window seconds, then --repeats such runs between two HIP events: their
median, min and max.
"""
import csv
import glob
import os
import statistics

SLEEP_PROBE_CYCLES = 10_000_000
_per_cycle = None                       # seconds per torch.cuda._sleep cycle, probed once per process


def hold_cycles(call_s, calls, per_cycle):
    """Sleep cycles that hold the stream while one window of ``calls`` calls is enqueued: at least 4x the slowest
    back-to-back window seen (``max(call_s)`` seconds per call x ``calls``), and at least 20 ms, so that the enqueue is
    over by a wide margin when the device starts to drain the queue.  ``per_cycle``: seconds per sleep cycle."""
    return int(max(4.0 * max(call_s) * calls, 0.02) / per_cycle)


def calls_for_window(seconds_per_call, window_s, floor):
    """Calls that fill ``window_s`` seconds at ``seconds_per_call``, never fewer than ``floor`` (a call below 0.1 us
    counts as 0.1 us)."""
    return max(floor, int(window_s / max(seconds_per_call, 1e-7)) + 1)


def _window(stream, enqueue, hold=0):
    """Seconds between two events around ``enqueue()`` on ``stream``, behind a sleep of ``hold`` cycles if any."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hold:
        torch.cuda._sleep(hold)
    a.record(stream)
    enqueue()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / 1e3


def _repeat(one, k):
    for _ in range(k):
        one()


def held(one, calls, boxes, warmup, stream=None):
    """(call_s, gpu_s): seconds per call of each of ``boxes`` windows of ``calls`` calls of ``one()``, back to back and
    behind a held stream.  ``one`` is invoked warmup + 2 x boxes x calls times, in this order: the warm-up, the
    back-to-back windows, the held windows (--trace-db of slice_time.py and slab_time.py counts on it)."""
    import torch

    global _per_cycle
    if stream is None:
        stream = torch.cuda.current_stream()
    if _per_cycle is None:
        _per_cycle = _window(stream, lambda: torch.cuda._sleep(SLEEP_PROBE_CYCLES)) / SLEEP_PROBE_CYCLES
    _repeat(one, warmup)
    call_s = [_window(stream, lambda: _repeat(one, calls)) / calls for _ in range(boxes)]
    hold = hold_cycles(call_s, calls, _per_cycle)
    gpu_s = [_window(stream, lambda: _repeat(one, calls), hold) / calls for _ in range(boxes)]
    torch.cuda.synchronize()
    return call_s, gpu_s


def timed(one, window_s, repeats, k0, warmup=None, stream=None):
    """(median, min, max, k): seconds per call of ``one()`` over ``repeats`` runs of k back-to-back calls, k sized to
    ``window_s`` seconds from a first run of ``k0`` calls after a warm-up of ``warmup`` calls (k0 when None: code
    objects, clocks).  ``one`` is invoked warmup + k0 + repeats x k times."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream()
    _repeat(one, k0 if warmup is None else warmup)
    k = calls_for_window(_window(stream, lambda: _repeat(one, k0)) / k0, window_s, k0)
    runs = [_window(stream, lambda: _repeat(one, k)) / k for _ in range(repeats)]
    return statistics.median(runs), min(runs), max(runs), k


def copy_seconds(nbytes, window_s, repeats, k0):
    """Median seconds of a device-to-device hipMemcpyAsync of ``nbytes`` bytes (it reads AND writes that many)."""
    import torch

    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src, non_blocking=True), window_s, repeats, k0)[0]


def kernel_stats(path, name_substrings, width):
    """The rows of every ``*kernel_stats.csv`` under ``path`` (a rocprofv3 --kernel-trace --stats run) whose kernel
    name holds one of ``name_substrings``, the name cut to ``width`` characters."""
    rows = []
    for name in sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)):
        with open(name) as f:
            for row in csv.DictReader(f):
                kernel = row.get("Name", "")
                if any(k in kernel for k in name_substrings):
                    rows.append({"file": os.path.relpath(name, path), "kernel": kernel[:width],
                                 "calls": int(row["Calls"]), "average_ms": round(float(row["AverageNs"]) / 1e6, 4),
                                 "min_ms": round(float(row["MinNs"]) / 1e6, 4),
                                 "max_ms": round(float(row["MaxNs"]) / 1e6, 4)})
    return rows


def c2_pairs(n, dev):
    """The three (density, labels) LODs of the BASELINE config 2 volume of edge ``n``, generated on ``dev``."""
    import torch

    from sub_volume_renderer_amd import synth

    pairs = [synth.volume(n, k, 4096, xp=torch, device=dev, slab=16) for k in range(3)]
    torch.cuda.synchronize()
    return pairs


def c2_scene(n, W, H, camera, storage=None, pairs=None, **spec_overrides):
    """(spec, scene) of BASELINE config 2 (bench.config2_spec) at ``W`` x ``H`` from ``camera``, built on cuda:0;
    ``storage``: the spec's ring_storage (None: its default), ``spec_overrides``: further fields of the spec set before
    the build.  (tools/prof_driver.py's build_scene pools its levels and is another scene.)"""
    import torch

    import bench
    from sub_volume_renderer_amd import testing

    spec = bench.config2_spec(n, W, H, camera, pairs if pairs is not None else c2_pairs(n, torch.device("cuda", 0)))
    if storage is not None:
        spec.ring_storage = storage
    for key, value in spec_overrides.items():
        setattr(spec, key, value)
    return spec, testing.build(spec)


def add_interpolation_argument(ap):
    ap.add_argument("--interpolation", default="nearest", choices=("nearest", "linear", "both"),
                    help="svr_set_interpolation mode of the timed calls; both: nearest and linear alternate, case by case")


def interpolations(choice):
    return ("nearest", "linear") if choice == "both" else (choice,)
