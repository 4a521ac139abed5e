"""A braking frame of the closed loop, two routes timed on the same GPU in ONE process, alternating call by call
(gaussianrpg_amd/closed_loop.py, csrc/ego_loop.hip).  One call is harness.closed_loop_step: render
the loop's next frame from its moved camera, detections_from_heads, the loop's step.
(a) device  closed_loop.EgoLoop: session.frame(k, camera=loop.camera) from the device row, one launch for ranging,
            command, ego step and the next camera row; nothing waits
(b) host    closed_loop.HostLoop, the route without the kernel and the baseline: session.frame(k, camera=(R, T)),
            one wait for det / count, the numpy tail, the Python dynamics
Both loops are commanded (policy=None) and braking from the first frame, so every frame is a moved camera.  The
repository ships no detector weights: the detector's heads are FIXED SYNTHETIC TENSORS (three levels of a
YOLOv5-shaped head, 80 classes, --boxes planted boxes that pass the thresholds), the same for every frame, and its
convolutions are not run.  Scenes: --background Gaussians and A = 10 and 50 actors of --actor-gaussians each at 1920 x 1280, max_det 10.
Per route: wall time of one call on the host with the device idle before it and waited for after it, median over
--steps calls, --reps times, the median of those medians with min and max; the host time from the call's entry to
the entry of the native frame call; the host synchronisations torch sees in one call.  Also: the step kernel's own
time by device events; the tail alone on a device `det` both ways, EgoLoop.step against the reference's tail as it is
written (count read back, then row by row over the DEVICE tensor: int() and torch.tensor() of 0-d device tensors,
each a wait), with the numpy ranging behind it.  No speed threshold belongs to this tool.  Prints one JSON line; --out
FILE also writes it (profiles/ego_loop_bench.json)."""
import argparse
import functools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import column, count_syncs, median, spread
from benchkit_scenes import ANCHORS, H, MAX_DET, NC, STRIDES, W, make_actors, make_models, make_tape, synthetic_heads
from gaussianrpg_amd import closed_loop as cl
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import rasterizer
from gaussianrpg_amd.perception import DetectGeometry, LetterboxPlan, detections_from_heads
from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
from gaussianrpg_amd.session import FrameSession


class FrontTimer:
    """wraps the binding's bound-frame function: perf_counter at its entry"""

    def __init__(self):
        self.at, self.C = None, rasterizer._C
        self.saved = self.C.rasterize_gaussians_bound_frame

    def __enter__(self):
        def g(*a, **kw):
            self.at = time.perf_counter()
            return self.saved(*a, **kw)
        self.C.rasterize_gaussians_bound_frame = g
        return self

    def __exit__(self, *exc):
        self.C.rasterize_gaussians_bound_frame = self.saved


def literal_tail(det, count, ranging):
    """the reference's tail on the device tensors as it is written: the count, then every row of the device tensor in
    turn -- int(cls), torch.tensor(xyxy) and .tolist() each wait for the device -- and distance() in numpy"""
    out = []
    gn = torch.tensor((ranging.H, ranging.W))[[1, 0, 1, 0]]
    for b, n in enumerate(count.tolist()):
        rows = det[b, :n]
        for row in reversed(rows):
            x1, y1, x2, y2, conf, cls = row
            if int(cls) not in ranging.class_ids:
                continue
            xyxy = torch.tensor([x1, y1, x2, y2]).view(1, 4)
            xywh = torch.stack([(xyxy[:, 0] + xyxy[:, 2]) / 2, (xyxy[:, 1] + xyxy[:, 3]) / 2, xyxy[:, 2] - xyxy[:, 0],
                                xyxy[:, 3] - xyxy[:, 1]], 1)
            xywh = (xywh / gn).view(-1).tolist()      # (the waits are what is timed; the ranging takes the box itself)
            box = np.concatenate([xyxy.view(-1).numpy(), [0.0, float(int(cls))]]).reshape(1, 6)
            out += list(cl.host_object_positions(box, ranging))
    return out


def timed(fn, steps, warmup=2):
    return median(column(benchkit.timed(fn, steps, warmup, events=False), "wall_us"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--actors", type=int, action="append")
    ap.add_argument("--background", type=int, default=1_900_000)
    ap.add_argument("--actor-gaussians", type=int, default=10_000)
    ap.add_argument("--tape", type=int, default=200)
    ap.add_argument("--boxes", type=int, default=10)
    args = ap.parse_args()
    benchkit.require_gpu("bench_ego_loop")
    dev = torch.device("cuda:0")
    T = args.tape
    result = {"bench": "tools/bench_ego_loop.py: one braking frame of the closed loop (render from the moved camera, "
                       "detections_from_heads, the loop's tail), closed_loop.EgoLoop (one launch, no wait) against "
                       "closed_loop.HostLoop (one wait, numpy tail, (R, T) to session.frame: the route without the kernel, "
                       "the baseline); us per call, wall on the host with the device idle before and waited for after, median "
                       "over %d calls, median / min / max of %d repetitions; the routes alternate call by call in one "
                       "process.  The detector's heads are fixed synthetic tensors (the repository ships no weights; "
                       "its convolutions are not run)." % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "width": W, "height": H, "background": args.background,
              "actor_gaussians": args.actor_gaussians, "tape_entries": T, "max_det": MAX_DET, "planted_boxes": args.boxes,
              "cases": {}}
    cam = hz.trajectory_camera(0, device=dev)
    settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))
    tape = make_tape(T)
    geom = DetectGeometry(np.asarray(ANCHORS, dtype=np.float32), STRIDES, NC)
    plan = LetterboxPlan.for_simulator(H, W)
    heads = synthetic_heads(dev, args.boxes)
    ranging = cl.Ranging.for_simulator(np.array([[1.0, 0, 0, 1.544414504251094167], [0, 1.0, 0, 0], [0, 0, 1.0, 2.1],
                                                 [0, 0, 0, 1.0]]), W, H)
    det, count = detections_from_heads(heads, geom, max_det=MAX_DET, plan=plan)
    torch.cuda.synchronize()
    result["detections_per_frame"] = int(count[0])
    for A in args.actors or [10, 50]:
        actors = make_actors(A, dev)
        models = make_models(A, args.background, args.actor_gaussians, dev, False)
        sc = hz.ClosedLoopScene(settings, models[0], models[1:], actors, tape, [(0, T - 1, 1.0)] * A)
        session = FrameSession(*sc[:6], **sc.options())
        kw = dict(policy=None, period=0.02, substeps=1)
        loops = {"device": cl.EgoLoop(session, ranging, steps=1 << 16, **kw), "host": cl.HostLoop(tape, ranging, **kw)}

        def call(route):
            loop = loops[route]
            if route == "device" and loop.num_steps >= loop.steps:
                loop.reset()
            return hz.closed_loop_step(session, loop, lambda frame: heads, geom, plan=plan, max_det=MAX_DET,
                                       command=-0.001)["rgb8"]
        for r in loops:                       # both brake from here on
            call(r)
        torch.cuda.synchronize()
        assert loops["device"].state()["activated"] == 1.0 and loops["host"].activated
        cell = {"A": A}
        meds = {r: [] for r in loops}
        routes = {r: functools.partial(call, r) for r in loops}
        for rep in range(args.reps):
            seen = benchkit.alternating(routes, args.steps, args.warmup if rep == 0 else 1, events=False)
            for r in loops:
                meds[r].append(round(median(column(seen[r], "wall_us")), 1))
        front = {r: [] for r in loops}
        with FrontTimer() as ft:
            for it in range(args.steps):
                for r in loops:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(r)
                    front[r].append((ft.at - t0) * 1e6)
        torch.cuda.synchronize()
        for r in loops:
            cell[r] = dict(spread(meds[r], prefix="wall_"), front_us=round(median(front[r]), 1),
                           host_syncs=count_syncs(lambda: call(r)))
        cell["host_minus_device_us"] = round(cell["host"]["wall_us"] - cell["device"]["wall_us"], 1)
        cell["spread_us"] = round(max(cell[r]["wall_max_us"] - cell[r]["wall_min_us"] for r in loops), 1)
        result["cases"]["A%d" % A] = cell
        if "tail" not in result:
            loop = loops["device"]
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 200
            loop.reset()
            loop.step(det, count, -0.001)
            torch.cuda.synchronize()
            start.record()
            for _ in range(n):
                loop.step(det, count, -0.001)
            stop.record()
            torch.cuda.synchronize()
            host = cl.HostLoop(tape, ranging, **kw)

            def host_tail():
                d = det.cpu().numpy()          # the one wait, as harness.closed_loop_step makes it
                host.step([rows[:int((rows[:, 4] > 0).sum())] for rows in d], -0.001)
            result["tail"] = {
                "what": "the tail alone on a device det / count of %d detections: us per call, wall with the device idle "
                        "before and waited for after (median of %d); kernel_us: %d back-to-back EgoLoop.step launches "
                        "between two device events, per launch (launch-bound: includes the gaps between launches)"
                        % (int(count[0]), args.steps, n),
                "kernel_us": round(start.elapsed_time(stop) * 1e3 / n, 2),
                "device_step_wall_us": round(timed(lambda: loop.step(det, count, -0.001), args.steps), 1),
                "host_loop_wall_us": round(timed(host_tail, args.steps), 1),
                "reference_as_written_wall_us": round(timed(lambda: literal_tail(det, count, ranging), args.steps), 1),
                "reference_as_written_host_syncs": count_syncs(lambda: literal_tail(det, count, ranging)),
                "host_loop_host_syncs": count_syncs(host_tail),
                "device_step_host_syncs": count_syncs(lambda: loop.step(det, count, -0.001))}
        del session, sc, loops, models, actors
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
