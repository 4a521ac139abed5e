"""Detector output -> detections (gaussianrpg_amd/perception.py, csrc/nms.hip): the simulator's
non_max_suppression + scale_coords(...).round() (simulator.py:349-368) on the detector's raw float32 [1,N,85] head
output, two routes timed on the same GPU in ONE process, alternating call by call:
(a) fused          harness.simulator_detections(fused=True): perception.detections (candidate pass, radix sort, one
                   greedy walk) and one host wait for the counts; "fused_no_wait" is perception.detections alone, which
                   is all a caller needs who consumes (det, count) on the device;
(b) torch          harness.simulator_detections(fused=False): the reference's lines in PyTorch on the device, with
                   torchvision.ops.nms (not installed on this stack) replaced by the IoU matrix on the device and the
                   greedy walk over it on the host.
Cases (nc = 80, candidates in clusters around objects as a detector's are):
  N = 25 200 (640 x 640 input), about 300 candidates, max_det 300
  N = 107 100 (the simulator's 1600 x 1088 input), about 3000 candidates, max_det 300 and the simulator's max_det 10
Per route and case: the time of one call between two device events, the host synchronised before and after (a call
of (b) waits on the host by itself), median over --steps calls, --reps times, median of those with the spread; the host
synchronisations torch sees in one call (sync debug mode).  The candidate pass's byte floor: the bytes it must touch
(every row's objectness, the class scores of the rows that pass the objectness test, one key and one class word per
row) at 8 TB/s; its achieved bytes/s needs the kernel's own time, from a run of its own,
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o stats -- python tools/bench_nms.py --only fused --case K
whose *kernel_stats.csv goes in with --kernel-stats K=FILE (repeatable) on the run that writes the result.
Prints one JSON line; --out FILE also writes it (profiles/nms_bench.json)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import count_syncs, spread
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.perception import LetterboxPlan, detections

NC = 80
# name -> (N, input (h, w), frame (H, W), candidates, objects, max_det)
CASES = {
    "N25200_c300": (25200, (640, 640), (640, 640), 300, 30, 300),
    "N107100_c3000": (107100, (1088, 1600), (1066, 1600), 3000, 100, 300),
    "N107100_c3000_maxdet10": (107100, (1088, 1600), (1066, 1600), 3000, 100, 10),
}
KERNELS = ("nms_candidates_kernel", "nms_walk_kernel", "radix_hist_kernel", "radix_digit_scan_kernel",
           "radix_scatter_kernel")


def make_prediction(N, size, n_cand, n_obj, seed):
    """float32 [1,N,5+NC] on the host: n_cand rows with obj > 0.5 and a best class score > 0.7, jittered around n_obj
    boxes; every other row has obj < 0.2 (conf_thres is 0.25)."""
    rng = np.random.RandomState(seed)
    p = np.zeros((1, N, 5 + NC), np.float32)
    p[0, :, 0] = rng.uniform(0, size[1], N)
    p[0, :, 1] = rng.uniform(0, size[0], N)
    p[0, :, 2:4] = rng.uniform(8, 200, (N, 2))
    p[0, :, 4] = rng.uniform(0.0, 0.2, N)
    p[0, :, 5:] = rng.uniform(0.0, 0.5, (N, NC))
    rows = np.sort(rng.choice(N, n_cand, replace=False))
    base = np.stack([rng.uniform(50, size[1] - 50, n_obj), rng.uniform(50, size[0] - 50, n_obj),
                     rng.uniform(30, 200, n_obj), rng.uniform(30, 200, n_obj)], axis=1)
    which = rng.randint(0, n_obj, n_cand)
    p[0, rows, :4] = base[which] + rng.uniform(-6, 6, (n_cand, 4))
    p[0, rows, 4] = rng.uniform(0.5, 1.0, n_cand)
    p[0, rows, 5:] = rng.uniform(0.0, 0.3, (n_cand, NC))
    p[0, rows, 5 + which % 8] = rng.uniform(0.7, 1.0, n_cand)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "fused"), default="all")
    ap.add_argument("--case", choices=list(CASES), action="append")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="CASE=FILE")
    args = ap.parse_args()
    benchkit.require_gpu("bench_nms")
    dev = torch.device("cuda:0")
    stats = dict(s.split("=", 1) for s in args.kernel_stats)
    result = {"bench": "tools/bench_nms.py: detector output -> detections in the frame, fused HIP against PyTorch on "
                       "the device with a host greedy walk; us per call between two device events, median over %d "
                       "calls, median of %d repetitions; the routes alternate in one process" % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "nc": NC, "cases": {}}
    for name in args.case or list(CASES):
        N, size, frame, n_cand, n_obj, max_det = CASES[name]
        plan = LetterboxPlan(frame[0], frame[1], size[1], device=dev)
        assert plan.out_shape == size, (plan, size)
        host = make_prediction(N, size, n_cand, n_obj, seed=N)
        pred = torch.from_numpy(host).to(dev)
        routes = {"fused_no_wait": lambda: detections(pred, max_det=max_det, plan=plan),
                  "fused": lambda: hz.simulator_detections(pred, plan, fused=True, max_det=max_det)}
        if args.only == "all":
            routes["torch"] = lambda: hz.simulator_detections(pred, plan, fused=False, max_det=max_det)
        kept = hz.simulator_detections(pred, plan, fused=True, max_det=max_det)[0]
        cell = {"N": N, "input": list(size), "frame": list(frame), "candidates": n_cand, "max_det": max_det,
                "kept": int(kept.shape[0])}
        if args.only == "all":
            other = hz.simulator_detections(pred, plan, fused=False, max_det=max_det)[0]
            cell["same_bits_as_torch_route"] = bool(other.shape == kept.shape and
                                                    torch.equal(other.view(torch.int32), kept.view(torch.int32)))
        # the candidate pass: 4 B of objectness per row, the class scores of the rows that pass it, 8 B written per row
        cell["candidate_pass_bytes"] = 4 * N + 4 * NC * n_cand + 8 * N
        cell["candidate_pass_floor_us_at_8TBs"] = cell["candidate_pass_bytes"] / 8e12 * 1e6
        cell["prediction_bytes"] = 4 * N * (5 + NC)
        reps = benchkit.windows(routes, args.reps, args.steps, args.warmup, wall=False)
        for k, fn in routes.items():
            cell[k] = dict(spread(reps[k]["device_us"]), host_syncs=count_syncs(fn))
        if args.only == "all":
            cell["torch_over_fused"] = cell["torch"]["us"] / cell["fused"]["us"]
        if name in stats:
            kt = benchkit.kernel_stats(stats[name], KERNELS)
            cell["kernels"] = kt
            if "nms_candidates_kernel" in kt:
                us = kt["nms_candidates_kernel"]["avg_us"]
                cell["candidate_pass_GBps"] = cell["candidate_pass_bytes"] / us / 1e3
                cell["candidate_pass_share_of_8TBs_floor"] = cell["candidate_pass_floor_us_at_8TBs"] / us
        result["cases"][name] = cell
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
