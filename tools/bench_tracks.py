"""Tracklets -> actor poses (gaussianrpg_amd/tracks.py, csrc/tracks.hip): the scene-graph part of
StreetGaussianModel.parse_camera (street_gaussian_model.py:239-283), two routes timed on the same GPU in ONE process,
alternating call by call:
(a) fused    harness.parse_camera_poses(fused=True): one launch for every actor, one gather of the visible rows;
(b) torch    harness.parse_camera_poses(fused=False): the reference's per-actor PyTorch with its host waits.
Cases: A = 10 and 50 actors, every track 198 entries long (F = 198, one column per actor), T = 1; evaluation (forward
under no_grad) and training (forward, a weighted sum of the poses as the loss, backward to opt_trans / opt_rots).
Per route and case: wall time of one call on the host, the device idle before it and waited for after it (what a
frame's first launch waits for), and the time between two device events around it; median over --steps calls,
--reps times, median of those with the spread.  Also the host synchronisations torch sees in one call (sync debug
mode) and the device kernels one call launches (torch.profiler; null where the profiler is not available).
No speed threshold belongs to this tool: the op is launch-sized, and the claim it measures is the launches and
waits it removes.  Prints one JSON line; --out FILE also writes it (profiles/tracks_bench.json)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import count_launches, count_syncs, median, spread
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.tracks import TrackTable, TrackedActorPoses

LENGTH = 198
BASE = 1.5e9


def make_turning_actors(A, dev, seed=0):
    """A actors on diverging, turning tracks (benchkit_scenes.make_actors is another scene: cars in rows ahead)"""
    rng = np.random.RandomState(seed)
    F = LENGTH
    tr = np.zeros((F, A, 8), np.float32)
    for a in range(A):
        yaw = 0.3 * a + 0.02 * np.arange(F) + rng.normal(0, 0.01, F)
        tr[:, a, 0] = a
        tr[:, a, 1:4] = np.stack([5.0 * a + 0.8 * np.arange(F), rng.normal(0, 0.1, F), np.full(F, 0.8)], 1)
        tr[:, a, 4], tr[:, a, 7] = np.cos(yaw / 2), np.sin(yaw / 2)
    stamps = BASE + 0.1 * np.arange(F)
    info = {a: dict(start_timestamp=stamps[0], end_timestamp=stamps[-1]) for a in range(A)}
    m = TrackedActorPoses(TrackTable.from_tracklets(tr, stamps, info), device=dev)
    with torch.no_grad():
        m.opt_trans.normal_(0, 0.05)
        m.opt_rots.normal_(0, 0.05)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--actors", type=int, action="append")
    args = ap.parse_args()
    benchkit.require_gpu("bench_tracks")
    dev = torch.device("cuda:0")
    result = {"bench": "tools/bench_tracks.py: parse_camera's actor poses, fused HIP against the reference's per-actor "
                       "PyTorch; us per call (wall on the host with the device idle before and waited for after, and "
                       "between two device events), median over %d calls, median of %d repetitions; the routes "
                       "alternate in one process" % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "list_length": LENGTH, "T": 1, "cases": {}}
    ego = torch.eye(4, device=dev)
    ego[:3, 3] = torch.tensor([3.0, -2.0, 0.5], device=dev)
    t = BASE + 0.1 * 77.3
    for A in args.actors or [10, 50]:
        m = make_turning_actors(A, dev)
        counts = [1000] * A
        g_rot, g_trans = torch.randn(A, 4, device=dev), torch.randn(A, 3, device=dev)

        def run(fused, train):
            if not train:
                with torch.no_grad():
                    return hz.parse_camera_poses(m, t, ego, counts, num_background=100000, fused=fused)[2:]
            m.zero_grad(set_to_none=True)
            rot, trans = hz.parse_camera_poses(m, t, ego, counts, num_background=100000, fused=fused)[2:]
            ((rot * g_rot).sum() + (trans * g_trans).sum()).backward()
            return m.opt_trans.grad, m.opt_rots.grad

        for mode, train in (("evaluation", False), ("training", True)):
            routes = {"fused": lambda: run(True, train), "torch": lambda: run(False, train)}
            a, b = run(True, train), run(False, train)
            cell = {"A": A, "max_abs_difference_between_routes": [float((x - y).abs().max()) for x, y in zip(a, b)]}
            reps = benchkit.windows(routes, args.reps, args.steps, args.warmup)
            for k, fn in routes.items():
                cell[k] = dict(spread(reps[k]["wall_us"], prefix="wall_"), device_events_us=median(reps[k]["device_us"]),
                               host_syncs=count_syncs(fn), launches=count_launches(fn))
            cell["torch_over_fused_wall"] = cell["torch"]["wall_us"] / cell["fused"]["wall_us"]
            result["cases"]["A%d_%s" % (A, mode)] = cell
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
