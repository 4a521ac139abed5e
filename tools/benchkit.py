"""How a call is timed by the side benches in tools/ (bench_*.py import this; the product, bench.py and the tests of
the product do not).  The method every tool states: routes alternate in one process, a warm-up precedes every timed
window, each window's figure is a median over its calls, and the repetitions are reported as median, min and max.

One window, `once`, is the only place a clock is read or an event recorded around a call:

    events made, synchronize | clock | event | out = fn(*args) | event | synchronize | clock | del out

`events` and `wall` switch the device-event pair and the host clock pair on and off: a launch-sized op is changed by an
Event.record() or a clock read inside its window, so a tool that reads one of the two asks for that one alone.  Whatever
a tool does per call in front of the window (`prepare`: fresh optimizers, cleared gradients) runs before the
synchronize.  `batch` is the same window around `inner` back-to-back calls whose results are dropped at once, per call.
All times are microseconds."""
import csv
import json
import os
import time
import warnings

import torch


def median(xs):
    """the upper median: what every recorded profile of these tools used (not statistics.median)"""
    return sorted(xs)[len(xs) // 2]


def require_gpu(tool):
    if not torch.cuda.is_available():
        raise SystemExit("%s: needs an MI355X (no ROCm device visible); nothing is measured without one" % tool)


def once(fn, *args, events=True, wall=True):
    """one call of fn(*args) in the window above: {"wall_us": host clock, "device_us": between the events}, each key
    only where its switch is on"""
    if events:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if wall:
        t0 = time.perf_counter()
    if events:
        e0.record()
    out = fn(*args)
    if events:
        e1.record()
    torch.cuda.synchronize()
    if wall:
        t1 = time.perf_counter()
    del out
    sample = {}
    if wall:
        sample["wall_us"] = (t1 - t0) * 1e6
    if events:
        sample["device_us"] = e0.elapsed_time(e1) * 1e3
    return sample


def batch(fn, inner, *, events=True):
    """`inner` back-to-back calls between two synchronises, per call: {"wall_us", "device_us" (events on)}"""
    if events:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if events:
        e0.record()
    for _ in range(inner):
        fn()
    if events:
        e1.record()
    torch.cuda.synchronize()
    sample = {"wall_us": (time.perf_counter() - t0) * 1e6 / inner}
    if events:
        sample["device_us"] = e0.elapsed_time(e1) * 1e3 / inner
    return sample


def timed(fn, steps, warmup, *, prepare=None, events=True, wall=True):
    """[sample of once] of `steps` calls after `warmup` untimed ones; with prepare, every call is fn(prepare()) and
    prepare runs in front of the window"""
    samples = []
    for it in range(warmup + steps):
        s = once(fn, *(() if prepare is None else (prepare(),)), events=events, wall=wall)
        if it >= warmup:
            samples.append(s)
    return samples


def alternating(routes, steps, warmup, *, inner=None, events=True, wall=True):
    """{route: [sample]}: the routes take turns call by call -- or, with inner, batch by batch"""
    samples = {k: [] for k in routes}
    for it in range(warmup + steps):
        for k, fn in routes.items():
            s = once(fn, events=events, wall=wall) if inner is None else batch(fn, inner, events=events)
            if it >= warmup:
                samples[k].append(s)
    return samples


def column(samples, key):
    return [s[key] for s in samples]


def medians(samples):
    """one window's figure: the median of each time the samples carry, {"wall_us", "device_us"}"""
    return {key: median(column(samples, key)) for key in samples[0]}


def windows(routes, reps, steps, warmup, *, again=1, **switches):
    """{route: {"wall_us" / "device_us": [each repetition's median]}}: per repetition one `timed` window per route, the
    routes taking turns window by window; the first repetition warms up with `warmup` calls, the later ones with
    `again`"""
    seen = {k: [] for k in routes}
    for r in range(reps):
        for k, fn in routes.items():
            seen[k].append(medians(timed(fn, steps, warmup if r == 0 else again, **switches)))
    return {k: {key: column(v, key) for key in v[0]} for k, v in seen.items()}


def spread(meds, unit="us", prefix=""):
    """the repetitions' medians as the tools write them: their median, min, max and the list itself"""
    return {prefix + unit: median(meds), prefix + "min_" + unit: min(meds), prefix + "max_" + unit: max(meds),
            prefix + "medians_" + unit: meds}


def count_syncs(fn):
    """Host synchronisations torch sees in one call (sync debug mode warns at each)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message).lower() for x in w)


def device_kernels(fn):
    """[(name, us)] of the device events (kernels, copies, memsets) of one call: one torch.profiler pass.  Raises where
    the profiler is not available; `optional` turns that into the tools' error record."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [(e.name, float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0))
            for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]


def optional(figure, *args):
    """figure(*args), or {"error": ...} where it raises: the profiler's figures are optional; the times are not"""
    try:
        return figure(*args)
    except Exception as e:
        return {"error": "%s: %s" % (type(e).__name__, e)}


def launch_counts(kernels):
    """device_kernels' list as {"kernels", "copies_and_memsets"}, or None where the profiler saw nothing"""
    if not kernels:
        return None
    copies = sum(("memcpy" in n.lower()) or ("memset" in n.lower()) for n, _ in kernels)
    return {"kernels": len(kernels) - copies, "copies_and_memsets": copies}


def count_launches(fn):
    """Device kernels (and memsets / copies apart) one call launches, None or an error record where the profiler
    cannot tell."""
    return optional(lambda: launch_counts(device_kernels(fn)))


def kernel_stats(path, names):
    """{short kernel name: {"avg_us", "calls"}} of a rocprofv3 --kernel-trace --stats kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in names:
                if k in r["Name"]:
                    out[k] = {"avg_us": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
    return out


def emit(result, out=None):
    """the tool's one JSON line; --out FILE gets the same document, indented"""
    print(json.dumps(result))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
