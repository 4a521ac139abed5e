"""Detector head -> detections (gaussianrpg_amd/perception.py, csrc/nms.hip): what the simulator does between its
detector's last convolutions and its detections -- the inference branch of Detect.forward (models/yolo.py:53-70), then
non_max_suppression + scale_coords(...).round() (simulator.py:349-368) -- on the nl conv outputs [1, 255, ny, nx],
three routes timed on the same GPU in ONE process, alternating call by call:
(a) torch_decode   harness.detect_inference_torch (the reference's lines in PyTorch on the device), then
                   perception.detections;
(b) decode_heads   perception.decode_heads (one launch, the [1,N,85] prediction), then perception.detections;
(c) from_heads     perception.detections_from_heads: the prediction never exists.
Cases (nc = 80, strides 8/16/32, candidates clustered around objects as a detector's are):
  N = 25 200 (640 x 640 input), about 300 candidates, max_det 300
  N = 107 100 (the simulator's 1600 x 1088 input), about 3000 candidates, max_det 300 and the simulator's max_det 10
Per route and case: the time of one call between two device events, the host synchronised before and after, median
over --steps calls, --reps times, median of those with the spread; the same for each stage of (a) and (b) on its own
(decode; detections on the finished prediction), and the host synchronisations torch sees in one call (sync debug
mode).  Route (a) keeps its grids and anchors on the device as the reference's module does (made by the first call,
outside the timed ones).  The bytes each route must move are computed from the shapes.  Kernel times need a run of
their own,
  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/bench_detect.py --only fused --reps 1 --case K
whose *kernel_trace.csv goes in with --kernel-trace K=FILE (repeatable) on the run that writes the result: per kernel
the median over its dispatches, the first KERNEL_WARMUP of them left out.
Prints one JSON line; --out FILE also writes it (profiles/detect_bench.json)."""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import count_syncs, median, spread
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.perception import DetectGeometry, LetterboxPlan, decode_heads, detections, detections_from_heads

NC = 80
STRIDES = (8, 16, 32)
ANCHORS = (((10, 13), (16, 30), (33, 23)), ((30, 61), (62, 45), (59, 119)), ((116, 90), (156, 198), (373, 326)))
# name -> (input (h, w), frame (H, W), candidates, objects, max_det)
CASES = {
    "N25200_c300": ((640, 640), (640, 640), 300, 30, 300),
    "N107100_c3000": ((1088, 1600), (1066, 1600), 3000, 100, 300),
    "N107100_c3000_maxdet10": ((1088, 1600), (1066, 1600), 3000, 100, 10),
}
KERNELS = ("detect_decode_kernel", "detect_candidates_kernel", "nms_candidates_kernel", "nms_walk_kernel",
           "radix_hist_kernel", "radix_digit_scan_kernel", "radix_scatter_kernel")


def make_heads(size, n_cand, n_obj, seed):
    """The three conv outputs float32 [1, 3*(5+NC), ny, nx] on the host: background objectness logits around -6 (no
    row passes conf_thres = 0.25), n_cand rows with an objectness logit in [0.5, 3] and one class logit in [1, 3], in
    cells around n_obj centres on every level, so their boxes overlap."""
    rng = np.random.RandomState(seed)
    no = 5 + NC
    heads = []
    for s in STRIDES:
        ny, nx = size[0] // s, size[1] // s
        h = rng.normal(0.0, 1.0, (1, 3 * no, ny, nx)).astype(np.float32)
        for a in range(3):
            h[0, a * no + 4] = rng.normal(-6.0, 0.7, (ny, nx)).clip(-12, -2)
            h[0, a * no + 5:(a + 1) * no] -= 3.0
        heads.append(h)
    centres = np.stack([rng.uniform(50, size[1] - 50, n_obj), rng.uniform(50, size[0] - 50, n_obj)], axis=1)
    seen = set()
    while len(seen) < n_cand:
        o = int(rng.randint(0, n_obj))
        l, a = int(rng.randint(0, 3)), int(rng.randint(0, 3))
        s = STRIDES[l]
        ny, nx = heads[l].shape[2:]
        x = int(np.clip(centres[o, 0] / s + rng.randint(-1, 2), 0, nx - 1))
        y = int(np.clip(centres[o, 1] / s + rng.randint(-1, 2), 0, ny - 1))
        if (l, a, y, x) in seen:
            continue
        seen.add((l, a, y, x))
        heads[l][0, a * no + 4, y, x] = rng.uniform(0.5, 3.0)
        heads[l][0, a * no + 5 + o % 8, y, x] = rng.uniform(1.0, 3.0)
    return heads


KERNEL_WARMUP = 5


def kernel_times(path):
    """{short kernel name: median / min / max us over its dispatches but the first KERNEL_WARMUP, and how many} of a
    rocprofv3 kernel_trace.csv"""
    durations = {k: [] for k in KERNELS}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    durations[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for k, d in durations.items():
        us = [(e - s) / 1e3 for s, e in sorted(d)[KERNEL_WARMUP:]]
        if us:
            out[k] = {"median_us": median(us), "min_us": min(us), "max_us": max(us), "dispatches": len(us)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "fused"), default="all", help="fused: routes (b) and (c) only")
    ap.add_argument("--case", choices=list(CASES), action="append")
    ap.add_argument("--kernel-trace", action="append", default=[], metavar="CASE=FILE")
    args = ap.parse_args()
    benchkit.require_gpu("bench_detect")
    dev = torch.device("cuda:0")
    stats = dict(s.split("=", 1) for s in args.kernel_trace)
    geom = DetectGeometry(np.asarray(ANCHORS, np.float32), STRIDES, NC)
    result = {"bench": "tools/bench_detect.py: detector conv outputs -> detections in the frame; (a) Detect's lines in "
                       "PyTorch then the fused NMS, (b) decode_heads then the fused NMS, (c) detections_from_heads; us "
                       "per call between two device events, median over %d calls, median of %d repetitions; the routes "
                       "alternate in one process; host_syncs: the host synchronisations torch sees in one call" %
                       (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "nc": NC, "cases": {}}
    for name in args.case or list(CASES):
        size, frame, n_cand, n_obj, max_det = CASES[name]
        plan = LetterboxPlan(frame[0], frame[1], size[1], device=dev)
        assert plan.out_shape == size, (plan, size)
        heads = [torch.from_numpy(h).to(dev) for h in make_heads(size, n_cand, n_obj, seed=size[0])]
        N = geom.rows(heads)
        kw = dict(max_det=max_det, plan=plan)
        pred_b = decode_heads(heads, geom)
        pred_a = hz.detect_inference_torch(heads, geom)
        routes = {"b_decode_heads": lambda: detections(decode_heads(heads, geom), **kw),
                  "c_from_heads": lambda: detections_from_heads(heads, geom, **kw)}
        stages = {"b_decode": lambda: decode_heads(heads, geom), "detections_on_pred": lambda: detections(pred_b, **kw)}
        if args.only == "all":
            routes = dict({"a_torch_decode": lambda: detections(hz.detect_inference_torch(heads, geom), **kw)}, **routes)
            stages["a_decode"] = lambda: hz.detect_inference_torch(heads, geom)
        det_c, count_c = detections_from_heads(heads, geom, **kw)
        det_b, count_b = detections(pred_b, **kw)
        det_a, count_a = detections(pred_a, **kw)
        unmapped = detections(pred_b, max_det=max_det)
        passed = int((pred_b[0, :, 4] > 0.25).sum())
        cell = {"N": N, "input": list(size), "frame": list(frame), "max_det": max_det, "kept": int(count_c[0]),
                "rows_past_objectness": passed,
                "b_and_c_same_bits": bool(torch.equal(det_b.view(torch.int32), det_c.view(torch.int32)) and
                                          torch.equal(count_b, count_c)),
                "a_and_c_same_count_and_classes": bool(torch.equal(count_a, count_c) and
                                                       torch.equal(det_a[..., 5], det_c[..., 5])),
                "a_and_c_max_abs_confidence_difference": float((det_a[..., 4] - det_c[..., 4]).abs().max()),
                "a_and_b_prediction_max_relative_difference":
                    float(((pred_a - pred_b).abs() / pred_b.abs().clamp(min=1e-30)).max()),
                "unmapped_kept": int(unmapped[1][0])}
        # bytes from the shapes.  The heads and the prediction are 4 * N * (5 + NC) bytes each.  decode_heads reads
        # the one and writes the other; the NMS candidate pass then reads 4 B per row and the class scores of the rows
        # past the objectness test and writes 8 B per row.  from_heads reads 4 B of objectness per row; a wave with a
        # row past the test reads the 4 + NC other planes of its 64 rows (256 B lines; counted as all 64 rows, an upper
        # bound when passing rows share a wave); it writes 8 B per row and 16 B per candidate.
        head_bytes = 4 * N * (5 + NC)
        cell["head_bytes"] = cell["prediction_bytes"] = head_bytes
        cell["b_bytes"] = 2 * head_bytes + 4 * N + 4 * NC * passed + 8 * N
        cell["c_bytes_upper"] = 4 * N + min(passed, (N + 63) // 64) * 64 * 4 * (4 + NC) + 8 * N + 16 * passed
        cell["b_floor_us_at_8TBs"] = cell["b_bytes"] / 8e12 * 1e6
        cell["c_floor_us_at_8TBs"] = cell["c_bytes_upper"] / 8e12 * 1e6
        both = dict(routes, **stages)
        reps = benchkit.windows(both, args.reps, args.steps, args.warmup, wall=False)
        for k, fn in both.items():
            cell[k] = dict(spread(reps[k]["device_us"]), host_syncs=count_syncs(fn))
        cell["b_over_c"] = cell["b_decode_heads"]["us"] / cell["c_from_heads"]["us"]
        if args.only == "all":
            cell["a_over_c"] = cell["a_torch_decode"]["us"] / cell["c_from_heads"]["us"]
            cell["a_over_b"] = cell["a_torch_decode"]["us"] / cell["b_decode_heads"]["us"]
        if name in stats:
            kt = kernel_times(stats[name])
            cell["kernels"] = kt
            if "detect_decode_kernel" in kt:
                cell["decode_kernel_GBps"] = 2 * head_bytes / kt["detect_decode_kernel"]["median_us"] / 1e3
        result["cases"][name] = cell
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
