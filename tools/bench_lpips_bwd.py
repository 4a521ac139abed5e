"""LPIPS as a training term (gaussianrpg_amd/lpips.py ``LPIPS.loss``, csrc/lpips_bwd.hip): forward + backward of one
pair at 1600 x 1066 and at 1920 x 1280, AlexNet and VGG16 with seeded weights (tests/lpips_truth.py); two routes timed on
the same GPU in ONE process, alternating call by call:
(a) torch   harness.lpips_torch(grad=True) under autograd: the vendor library's convolutions and their backward, one
            launch for every elementwise step of both directions -- the baseline; warmed up until two successive calls
            agree within 5 % (the library's first-call searches)
(b) native  LPIPS.loss and its backward: two native calls, 13 + 12 (AlexNet) / 23 + 22 (VGG16) launches
Per route: wall time of one forward + backward on the host with the device idle before it and waited for after it,
median over --steps calls, --reps times, the median of those medians with min and max; the device launches (torch
profiler).  For (b) the training workspace's bytes next to the metric's.  --routes b measures (b) alone.  No speed
threshold belongs to this tool.  Prints one JSON line; --out FILE also writes it (profiles/lpips_bwd_bench.json)."""
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
from benchkit import column, median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import lpips as LP

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
    benchkit.require_gpu("bench_lpips_bwd")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": "seeded weights, one pair, forward + backward to x",
           "routes": args.routes, "steps": args.steps, "reps": args.reps,
           "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE"), "nets": {}}
    for net in args.net or ["alex", "vgg"]:
        features, lin = T.build_features(net), T.build_lin(net)
        crit = LP.LPIPS(net, features, lin)
        tnet = hz.lpips_torch(net, features, lin, device=dev, grad=True) if args.routes == "ab" else None
        res["nets"][net] = {}
        for name in args.size or list(SIZES):
            h, w = SIZES[name]
            x, y = (torch.from_numpy(a).to(dev) for a in T.build_pair(1, h, w, 5))
            x.requires_grad_(True)
            ones = torch.ones(1, device=dev)

            def native():
                return torch.autograd.grad(crit.loss(x, y), x, ones)[0]

            def vendor():
                return torch.autograd.grad(tnet(x, y).sum(), x)[0]

            routes = {"native": native}
            P = LP.shape_plan(net, 1, h, w)
            train_bytes = LP._C().lpips_train_workspace_bytes(LP.NETS[net], 1, h, w)
            row = {"input": [1, 3, h, w], "train_workspace_bytes": train_bytes, "train_workspace_mib": train_bytes / 2 ** 20,
                   "metric_workspace_bytes": P["workspace_bytes"],
                   "planned_launches": {"forward": P["launches"]["total"], "backward": P["backward_launches"]["total"]}}
            if tnet is not None:
                routes["torch"] = vendor
                t0 = time.perf_counter()
                prev, settle = None, []
                for _ in range(30):
                    t = median(wall(vendor, 1))
                    settle.append(t)
                    if prev is not None and abs(t - prev) <= 0.05 * prev:
                        break
                    prev = t
                row["torch_warmup_calls_ms"], row["torch_warmup_s"] = settle, time.perf_counter() - t0
                a, b = native().double(), vendor().double()
                row["gradient_relative_l2_between_routes"] = float(torch.linalg.norm(a - b) / torch.linalg.norm(b))
            wall(native, 3)
            meds = {r: [] for r in routes}
            for _ in range(args.reps):
                seen = benchkit.alternating(routes, args.steps, 0, events=False)
                for r in routes:
                    meds[r].append(median(column(seen[r], "wall_us")) / 1e3)
            for r, fn in routes.items():
                row[r] = {"wall_ms": median(meds[r]), "min": min(meds[r]), "max": max(meds[r]),
                          "launches": benchkit.optional(lambda: len(benchkit.device_kernels(fn)))}
            if tnet is not None:
                row["native_over_torch"] = row["native"]["wall_ms"] / row["torch"]["wall_ms"]
            res["nets"][net][name] = row
            print(net, name, {r: row[r]["wall_ms"] for r in routes}, file=sys.stderr)
            del x, y
        del crit, tnet
        torch.cuda.empty_cache()
    benchkit.emit(res, args.out)


if __name__ == "__main__":
    main()
