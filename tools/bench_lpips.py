"""LPIPS (gaussianrpg_amd/lpips.py, csrc/lpips.hip): one pair at 1600 x 1066 and at 1920 x 1280, AlexNet and VGG16 with
seeded weights (tests/lpips_truth.py); two routes timed on the same GPU in ONE process, alternating call by call:
(a) torch   harness.lpips_torch on the device: the vendor library's convolutions plus one launch for every z-score step,
            ReLU, pool, normalisation, difference, 1 x 1 convolution and mean -- the baseline; warmed up until two
            successive calls agree within 5 % (the library's first-call searches)
(b) native  lpips.LPIPS.distances: one native call, 13 (AlexNet) / 23 (VGG16) launches
Per route: wall time of one call on the host with the device idle before it and waited for after it, median over
--steps calls, --reps times, the median of those medians with min and max; the device launches (torch profiler) and the
host synchronisations torch sees in one call (sync debug mode).  For (b) the workspace ("arena") bytes and the
convolutions' FLOPs 2 M N K over the wall time.  --routes b measures (b) alone.  No speed threshold belongs to this tool.
Prints one JSON line; --out FILE also writes it (profiles/lpips_bench.json)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import benchkit
import lpips_truth as T
from benchkit import column, count_syncs, median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import lpips as LP

PEAK_F32_MATRIX = 157.3e12
SIZES = {"1600x1066": (1066, 1600), "1920x1280": (1280, 1920)}


def wall(fn, steps):
    """ms per call, wall on the host, of `steps` calls"""
    return [us / 1e3 for us in column(benchkit.timed(fn, steps, 0, events=False), "wall_us")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--routes", default="ab", choices=["ab", "b"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", action="append", choices=list(SIZES))
    ap.add_argument("--net", action="append", choices=["alex", "vgg"])
    args = ap.parse_args()
    benchkit.require_gpu("bench_lpips")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": "seeded weights, one pair", "routes": args.routes,
           "steps": args.steps, "reps": args.reps, "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE"), "nets": {}}
    for net in args.net or ["alex", "vgg"]:
        features, lin = T.build_features(net), T.build_lin(net)
        crit = LP.LPIPS(net, features, lin)
        tnet = hz.lpips_torch(net, features, lin, device=dev) if args.routes == "ab" else None
        res["nets"][net] = {}
        for name in args.size or list(SIZES):
            h, w = SIZES[name]
            x, y = (torch.from_numpy(a).to(dev) for a in T.build_pair(1, h, w, 5))
            routes = {"native": lambda: crit.distances(x, y)}
            P = LP.shape_plan(net, 1, h, w)
            flops = sum(2 * s["c_out"] * 2 * s["hw_out"][0] * s["hw_out"][1] * s["c_in"] * s["k"] ** 2
                        for s in P["steps"] if s["kind"] == "conv")
            row = {"input": [1, 3, h, w], "arena_bytes": P["workspace_bytes"], "arena_mib": P["workspace_bytes"] / 2 ** 20,
                   "gflop": flops / 1e9, "planned_launches": P["launches"]}
            if tnet is not None:
                routes["torch"] = lambda: tnet(x, y)
                t0 = time.perf_counter()
                prev, settle = None, []
                for _ in range(30):
                    t = median(wall(routes["torch"], 1))
                    settle.append(t)
                    if prev is not None and abs(t - prev) <= 0.05 * prev:
                        break
                    prev = t
                row["torch_warmup_calls_ms"], row["torch_warmup_s"] = settle, time.perf_counter() - t0
                a, b = float(crit(x, y)), float(tnet(x, y))
                row["values"] = {"native": a, "torch": b, "relative_difference": abs(a - b) / abs(b)}
            wall(routes["native"], 3)
            meds = {r: [] for r in routes}
            for _ in range(args.reps):
                seen = benchkit.alternating(routes, args.steps, 0, events=False)
                for r in routes:
                    meds[r].append(median(column(seen[r], "wall_us")) / 1e3)
            for r, fn in routes.items():
                row[r] = {"wall_ms": median(meds[r]), "min": min(meds[r]), "max": max(meds[r]),
                          "launches": benchkit.optional(lambda: len(benchkit.device_kernels(fn))), "host_syncs": count_syncs(fn)}
            row["native"]["tflops_over_wall"] = flops / (row["native"]["wall_ms"] * 1e-3) / 1e12
            row["native"]["share_of_f32_matrix_peak"] = flops / (row["native"]["wall_ms"] * 1e-3) / PEAK_F32_MATRIX
            res["nets"][net][name] = row
            print(net, name, {r: row[r]["wall_ms"] for r in routes}, file=sys.stderr)
            del x, y
        del crit, tnet
        torch.cuda.empty_cache()
    benchkit.emit(res, args.out)


if __name__ == "__main__":
    main()
