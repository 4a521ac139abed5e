"""Tracked actor poses into a composed frame, two hand-overs timed on the same GPU in ONE process, alternating call by
call (gaussianrpg_amd/tracks.py, gaussianrpg_amd/composed.py, csrc/segment_pose.hip):
(a) table   harness.tracked_poses(device_poses=True):  PoseBatch.rows -> PoseTable; the library's segment table takes the
            poses from device memory on the frame's stream (grpg_bind_device_poses)
(b) rows    harness.tracked_poses(device_poses=False): PoseBatch.frame -> PoseRows; four small launches and one
            device-to-host copy in front of the frame -- the parent commit's route, unchanged
Cases: A = 10 and 50 actors of --actor-gaussians Gaussians behind --background background ones, every track 198 entries
long; the evaluation frame (harness.tracked_simulator_frame: actors.poses + forward_frame, rgb8) and the training step
(harness.tracked_train_step: actors.poses + training forward + backward to the raw parameters and opt_trans / opt_rots).
Per route and case: wall time of one call on the host with the device idle before it and waited for after it, median
over --steps calls, --reps times; the median of those medians, their spread, and the host synchronisations torch sees in
one call (sync debug mode).  The two routes' frames are compared byte for byte first.
No speed threshold belongs to this tool.  Prints one JSON line; --out FILE also writes it
(profiles/device_poses_bench.json)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from benchkit import column, count_syncs, median, spread
from benchkit_scenes import BASE, LENGTH, make_actors, make_models
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import ComposedRasterizer
from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--actors", type=int, action="append")
    ap.add_argument("--background", type=int, default=200_000)
    ap.add_argument("--actor-gaussians", type=int, default=2_000)
    args = ap.parse_args()
    benchkit.require_gpu("bench_device_poses")
    dev = torch.device("cuda:0")
    result = {"bench": "tools/bench_device_poses.py: tracked actor poses into a composed frame, PoseTable (device rows, "
                       "grpg_bind_device_poses) against PoseRows (the host hand-over); us per call, wall on the host with "
                       "the device idle before and waited for after, median over %d calls, median of %d repetitions; the "
                       "routes alternate call by call in one process" % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "list_length": LENGTH, "background": args.background,
              "actor_gaussians": args.actor_gaussians, "cases": {}}
    cam = hz.trajectory_camera(0, device=dev)
    rast = ComposedRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1)))
    ego = torch.eye(4, device=dev)
    ego[:3, 3] = torch.tensor([0.3, -0.2, 0.5], device=dev)
    t = BASE + 0.1 * 77.3
    for A in args.actors or [10, 50]:
        actors = make_actors(A, dev)
        visible = list(range(A))
        times = [0.1 + 0.01 * a for a in visible]
        for mode in ("evaluation", "training"):
            train = mode == "training"
            models = make_models(A, args.background, args.actor_gaussians, dev, train)
            params = [p for m in models for p in m[:6]] + list(actors.parameters())

            def call(device_poses):
                if not train:
                    return hz.tracked_simulator_frame(rast, models, actors, t, ego, visible, times,
                                                      device_poses=device_poses)["rgb8"]
                for p in params:
                    p.grad = None
                return hz.tracked_train_step(rast, models, actors, t, ego, visible, times, device_poses=device_poses)

            routes = {"table": lambda: call(True), "rows": lambda: call(False)}
            a, b = call(True).clone(), call(False).clone()
            cell = {"A": A, "frames_equal": bool(torch.equal(a, b))}
            meds = {k: [] for k in routes}
            for r in range(args.reps):
                seen = benchkit.alternating(routes, args.steps, args.warmup if r == 0 else 1, events=False)
                for k in routes:
                    meds[k].append(median(column(seen[k], "wall_us")))
            for k, fn in routes.items():
                cell[k] = dict(spread([round(x, 1) for x in meds[k]], prefix="wall_"), host_syncs=count_syncs(fn))
            cell["rows_minus_table_us"] = round(cell["rows"]["wall_us"] - cell["table"]["wall_us"], 1)
            cell["rows_spread_us"] = round(cell["rows"]["wall_max_us"] - cell["rows"]["wall_min_us"], 1)
            result["cases"]["A%d_%s" % (A, mode)] = cell
            del models, params
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
