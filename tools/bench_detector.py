"""The detector's network (gaussianrpg_amd/detector.py, csrc/detector.hip): yolov5s, nc 80, seeded weights
(tests/detector_truth.py), bs 1, at the simulator's 1600 x 1088 input and at 1920 x 1280; two routes timed on the same
GPU in ONE process, alternating call by call:
(a) torch   harness.detector_torch on the device with fused weights: the vendor library's convolutions plus one launch
            for every SiLU, cat, shortcut add, max-pool and upsample -- the baseline; warmed up until two successive
            calls agree within 5 % (the library's first-call searches)
(b) native  detector.DetectorNet: one native call, 63 launches
Per route: wall time of one call on the host with the device idle before it and waited for after it, median over
--steps calls, --reps times, the median of those medians with min and max; the device launches (torch profiler) and
the host synchronisations torch sees in one call (sync debug mode).  For (b): the device time of every launch on its
own between two events (median of --layer-reps), its FLOPs 2 M N K, and the achieved FLOP/s of the whole list as a
share of the 157 TFLOP/s f32 matrix peak.  --routes b measures (b) alone (a machine whose vendor library cannot run a
layer).  --closed-loop adds the braking frame of tools/bench_ego_loop.py (1.9 M + 10 x 10 k Gaussians at 1920 x 1280,
closed_loop.EgoLoop, commanded braking, max_det 10) with three things in harness.closed_loop_step's heads slot,
alternating call by call: that tool's fixed synthetic heads (no network: the parent's figure and the baseline), route
(a) and route (b) behind perception.detector_input.  --half adds the fp16 rows to the same alternation (DESIGN.md section
31): native_f16, DetectorNet(dtype=torch.float16) on a half input (csrc/detector_f16.hip; its share is of the f16 matrix
peak, 16 x the f32 one), and -- with route (a) -- torch_f16, harness.detector_torch(dtype=torch.float16) on the device
with the float32-fused weights rounded to half, warmed up the same way; with --closed-loop also the braking frame with
each of them behind detector_input(..., dtype=torch.float16) (profiles/detector_f16_bench.json).  No speed threshold
belongs to this tool.  Prints one JSON line; --out FILE also writes it (profiles/detector_bench.json)."""
import argparse
import functools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import benchkit
import detector_truth as T
from benchkit import column, count_syncs, median
from gaussianrpg_amd import detector as D
from gaussianrpg_amd import harness as hz

PEAK_F32_MATRIX = 157.3e12
PEAK_F16_MATRIX = 16 * PEAK_F32_MATRIX
SIZES = {"1600x1088": (1088, 1600), "1920x1280": (1280, 1920)}


def wall(fn, steps):
    """ms per call, wall on the host, of `steps` calls"""
    return [us / 1e3 for us in column(benchkit.timed(fn, steps, 0, events=False), "wall_us")]


def alternating_wall(routes, steps, reps):
    """{route: [each repetition's median wall us]}: the routes alternate call by call"""
    meds = {r: [] for r in routes}
    for _ in range(reps):
        seen = benchkit.alternating(routes, steps, 0, events=False)
        for r in routes:
            meds[r].append(median(column(seen[r], "wall_us")))
    return meds


def per_layer(net, P, reps):
    rows = []
    spec_convs = net.spec.convs()
    for n, s in enumerate(P.steps):
        rec = P.records[n:n + 1].clone()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            (D.run_records_f16 if net.dtype == torch.float16 else D.run_records)(rec, P.arena)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        row = {"kind": s["kind"], "ms": median(ts)}
        if s["kind"] == "conv":
            ho, wo = s["hw_out"]
            row.update(key=s["key"], M=s["c_out"], N=P.bs * ho * wo, K=s["c_in"] * s["k"] ** 2,
                       tile=128 if s["tile"] == D.TILE_128 else 64)
            row["flops"] = 2 * row["M"] * row["N"] * row["K"]
            row["tflops"] = row["flops"] / (row["ms"] * 1e-3) / 1e12
        rows.append(row)
    return rows


def closed_loop_frame(dev, routes_of, steps, reps):
    """us per braking frame for every entry of routes_of(plan) -> {name: heads_of(frame)}."""
    import numpy as np
    import benchkit_scenes as be
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from gaussianrpg_amd import closed_loop as cl
    from gaussianrpg_amd.perception import LetterboxPlan
    from gaussianrpg_amd.session import FrameSession
    A, tape_len = 10, 200
    cam = hz.trajectory_camera(0, device=dev)
    settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))
    tape = be.make_tape(tape_len)
    plan = LetterboxPlan.for_simulator(be.H, be.W)
    ranging = cl.Ranging.for_simulator(np.array([[1.0, 0, 0, 1.544414504251094167], [0, 1.0, 0, 0], [0, 0, 1.0, 2.1],
                                                 [0, 0, 0, 1.0]]), be.W, be.H)
    actors = be.make_actors(A, dev)
    models = be.make_models(A, 1_900_000, 10_000, dev, False)
    sc = hz.ClosedLoopScene(settings, models[0], models[1:], actors, tape, [(0, tape_len - 1, 1.0)] * A)
    session = FrameSession(*sc[:6], **sc.options())
    routes, geom = routes_of(plan, be.synthetic_heads(dev, 10))
    loops = {r: cl.EgoLoop(session, ranging, steps=1 << 16, policy=None, period=0.02, substeps=1) for r in routes}

    def call(r):
        return hz.closed_loop_step(session, loops[r], routes[r], geom, plan=plan, max_det=be.MAX_DET, command=-0.001)["rgb8"]
    for _ in range(4):
        for r in routes:
            call(r)
    meds = alternating_wall({r: functools.partial(call, r) for r in routes}, steps, reps)
    out = {"scene": "1.9 M + 10 x 10 k Gaussians, 1920 x 1280, detector input %s" % (list(plan.out_shape),)}
    for r in routes:
        out[r] = {"wall_us": median(meds[r]), "min": min(meds[r]), "max": max(meds[r]), "host_syncs": count_syncs(lambda: call(r))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--closed-loop", action="store_true")
    ap.add_argument("--routes", default="ab", choices=["ab", "b"])
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layer-reps", type=int, default=5)
    ap.add_argument("--size", action="append", choices=list(SIZES))
    args = ap.parse_args()
    benchkit.require_gpu("bench_detector")
    dev = torch.device("cuda:0")
    spec = T.spec_of(False)
    sd = T.build_weights(spec, 12)
    net = D.DetectorNet(spec, sd)
    fused = {}
    for c, (w, b) in zip(spec.convs(), net.params):
        pre = c["key"] + ("" if c["plain"] else ".conv")
        fused[pre + ".weight"], fused[pre + ".bias"] = w, b
    net16 = D.DetectorNet(spec, sd, dtype=torch.float16) if args.half else None
    res = {"device": torch.cuda.get_device_name(0), "model": "yolov5s nc 80, seeded weights, bs 1", "routes": args.routes,
           "half": args.half,
           "steps": args.steps, "reps": args.reps, "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE"), "sizes": {}}
    for name in args.size or list(SIZES):
        h, w = SIZES[name]
        x = torch.from_numpy(T.build_input(1, h, w, 5)).to(dev)
        routes = {"native": lambda: net(x)}
        nets = {"native": net}
        row = {"input": [1, 3, h, w]}
        if args.half:
            xh = x.half()
            routes["native_f16"] = lambda: net16(xh)
            nets["native_f16"] = net16

        def settle_torch(name, suffix=""):
            t0 = time.perf_counter()
            prev, settle = None, []
            for _ in range(30):
                t = median(wall(routes[name], 1))
                settle.append(t)
                if prev is not None and abs(t - prev) <= 0.05 * prev:
                    break
                prev = t
            row["torch%s_warmup_calls_ms" % suffix] = settle
            row["torch%s_warmup_s" % suffix] = time.perf_counter() - t0
        if args.routes == "ab":
            tnet = hz.detector_torch(spec, fused, device=dev)
            routes["torch"] = lambda: tnet(x)
            settle_torch("torch")
            ht, hn = tnet(x), net(x)
            row["routes_rel_l2"] = [T.rel_l2(a.cpu(), b.cpu()) for a, b in zip(hn, ht)]
            if args.half:
                tnet16 = hz.detector_torch(spec, fused, dtype=torch.float16, device=dev)
                routes["torch_f16"] = lambda: tnet16(xh)
                settle_torch("torch_f16", "_f16")
                row["routes_f16_rel_l2"] = [T.rel_l2(a.cpu(), b.float().cpu()) for a, b in zip(net16(xh), tnet16(xh))]
                row["native_f16_from_native_rel_l2"] = [T.rel_l2(a.cpu(), b.cpu()) for a, b in zip(net16(xh), net(x))]
        for r in nets:
            wall(routes[r], 3)
        meds = {r: [us / 1e3 for us in v] for r, v in alternating_wall(routes, args.steps, args.reps).items()}
        for r, fn in routes.items():
            row[r] = {"wall_ms": median(meds[r]), "min": min(meds[r]), "max": max(meds[r]),
                      "launches": len(benchkit.device_kernels(fn)), "host_syncs": count_syncs(fn)}
        for r, n in nets.items():
            P = n.plan(1, h, w, dev)
            layers = per_layer(n, P, args.layer_reps)
            flops = sum(l.get("flops", 0) for l in layers)
            dev_ms = sum(l["ms"] for l in layers)
            half = n.dtype == torch.float16
            row[r].update({"arena_mib": P.arena_bytes / 2 ** 20, "gflop": flops / 1e9, "sum_of_layer_ms": dev_ms,
                           "tflops_over_wall": flops / (row[r]["wall_ms"] * 1e-3) / 1e12,
                           "share_of_f16_matrix_peak" if half else "share_of_f32_matrix_peak":
                               flops / (row[r]["wall_ms"] * 1e-3) / (PEAK_F16_MATRIX if half else PEAK_F32_MATRIX),
                           "tile128_layers": sum(l.get("tile") == 128 for l in layers), "layers": layers})
        res["sizes"][name] = row
        print(name, {r: row[r]["wall_ms"] for r in routes}, file=sys.stderr)
    if args.closed_loop:
        from gaussianrpg_amd.perception import detector_input

        def routes_of(plan, synthetic):
            r = {"synthetic_heads": lambda frame: synthetic,
                 "native": lambda frame: net(detector_input(frame["rgb8"], plan))}
            if args.routes == "ab":
                tnet = hz.detector_torch(spec, fused, device=dev)
                r["torch"] = lambda frame: tnet(detector_input(frame["rgb8"], plan))
            if args.half:
                r["native_f16"] = lambda frame: net16(detector_input(frame["rgb8"], plan, dtype=torch.float16))
                if args.routes == "ab":
                    tnet16 = hz.detector_torch(spec, fused, dtype=torch.float16, device=dev)
                    r["torch_f16"] = lambda frame: [h.float() for h in tnet16(detector_input(frame["rgb8"], plan,
                                                                                            dtype=torch.float16))]
            return r, net.geometry
        res["closed_loop_frame"] = closed_loop_frame(dev, routes_of, args.steps, args.reps)
        print("closed loop", {k: v["wall_us"] for k, v in res["closed_loop_frame"].items() if isinstance(v, dict)}, file=sys.stderr)
    benchkit.emit(res, args.out)


if __name__ == "__main__":
    main()
