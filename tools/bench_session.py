"""The closed loop's frame, two routes timed on the same GPU in ONE process, alternating call by call
(gaussianrpg_amd/session.py, csrc/frame_table.hip):
(a) bound    harness.closed_loop_frame(bound=True): session.FrameSession bound once to the scene and the tape, then
             session.frame(k, camera) -- the segment tables of all frames baked on the device (grpg_frame_tables_bake),
             the frame call reads its rows in place (grpg_bind_frame_table)
(b) unbound  harness.closed_loop_frame(bound=False): per frame the visible list and the Fourier times, a device camera
             (make_camera(..., device=dev)) and its settings object, tracked_simulator_frame(device_poses=True) -- the
             pose launch, the packing, the table upload, the pose gather -- and ray_matrix_host: the parent commit's
             code, the baseline
Scenes: --background Gaussians and A = 10 and 50 actors of --actor-gaussians each at 1920 x 1280, a tape of --tape
entries with every actor visible.  Cases: the tape's own camera; a moved camera ((R, T) per frame); sky composite with
the bytes delivered to pinned host memory.  Per route and case: wall time of one call on the host with the device idle
before it and waited for after it, median over --steps calls, --reps times; the median of those medians and their
spread; the host time from the call's entry to the entry of the native frame call (everything the route does in front
of the library's first launch of the frame, measured by wrapping the binding's function; the unbound route's pose
launch lies inside that span); the host synchronisations torch sees in one call; and the bind time of the session.
The two routes' frames are compared byte for byte first.  No speed threshold belongs to this tool.  Prints one JSON
line; --out FILE also writes it (profiles/session_bench.json)."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import count_syncs, median, spread
from benchkit_scenes import H, W, make_actors, make_models, make_tape
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import rasterizer
from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
from gaussianrpg_amd.session import FrameSession


def moved(k):
    yaw = 0.01 * math.sin(0.1 * k) + 0.004 * math.cos(0.7 * k)
    R = np.array([[math.cos(yaw), 0.0, math.sin(yaw)], [0.0, 1.0, 0.0], [-math.sin(yaw), 0.0, math.cos(yaw)]])
    C = np.array([0.05 * math.sin(k), 0.0, 0.02 * k + 0.03])
    return R, -R.transpose() @ C


class FrontTimer:
    """wraps the binding's two frame functions: perf_counter at their entry"""

    def __init__(self):
        self.at = None
        self.C = rasterizer._C
        self.saved = {n: getattr(self.C, n) for n in ("rasterize_gaussians_composed_frame", "rasterize_gaussians_bound_frame")}

    def __enter__(self):
        for n, f in self.saved.items():
            setattr(self.C, n, self._wrap(f))
        return self

    def _wrap(self, f):
        def g(*a, **kw):
            self.at = time.perf_counter()
            return f(*a, **kw)
        return g

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(self.C, n, f)


def timed_alternating(routes, steps, warmup, T):
    """{route: [wall us per call]}: the routes take turns, call by call, on the same frame of the tape"""
    wall = {r: [] for r in routes}
    for it in range(warmup + steps):
        k = (7 * it) % T
        for r, fn in routes.items():
            s = benchkit.once(fn, k, events=False)
            if it >= warmup:
                wall[r].append(s["wall_us"])
    return wall


def front_times(routes, steps, T):
    """{route: median us from the call's entry to the entry of the native frame call}"""
    out = {r: [] for r in routes}
    with FrontTimer() as ft:
        for it in range(steps):
            k = (7 * it) % T
            for r, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(k)
                out[r].append((ft.at - t0) * 1e6)
    torch.cuda.synchronize()
    return {r: round(median(v), 1) for r, v in out.items()}


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
    args = ap.parse_args()
    benchkit.require_gpu("bench_session")
    dev = torch.device("cuda:0")
    T = args.tape
    result = {"bench": "tools/bench_session.py: the closed loop's frame, FrameSession (bound once: baked segment tables, "
                       "grpg_bind_frame_table) against the per-frame route (closed_loop_frame(bound=False), the parent "
                       "commit's code: the baseline); us per call, wall on the host with the device idle before and waited "
                       "for after, median over %d calls, median of %d repetitions; the routes alternate call by call in "
                       "one process; front_us: host time from the call's entry to the entry of the native frame call"
                       % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "width": W, "height": H, "background": args.background,
              "actor_gaussians": args.actor_gaussians, "tape_entries": T, "cases": {}}
    cam = hz.trajectory_camera(0, device=dev)
    settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))
    tape = make_tape(T)
    sky = torch.rand(6, 256, 256, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    pinned = torch.empty(H, W, 3, dtype=torch.uint8).pin_memory()
    for A in args.actors or [10, 50]:
        actors = make_actors(A, dev)
        models = make_models(A, args.background, args.actor_gaussians, dev, False)
        spans = [(0, T - 1, 1.0)] * A
        for case in ("tape_camera", "moved_camera", "sky_pinned_host"):
            opts = dict(sky_cube=sky) if case == "sky_pinned_host" else {}
            sc = hz.ClosedLoopScene(settings, models[0], models[1:], actors, tape, spans, **opts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            session = FrameSession(*sc[:6], **sc.options())
            torch.cuda.synchronize()
            bind_ms = (time.perf_counter() - t0) * 1e3
            camera = moved if case == "moved_camera" else (lambda k: None)
            kw = dict(out=pinned) if case == "sky_pinned_host" else {}
            routes = {"bound": lambda k: hz.closed_loop_frame(sc, k, camera(k), bound=True, session=session, **kw)["rgb8"],
                      "unbound": lambda k: hz.closed_loop_frame(sc, k, camera(k), bound=False, **kw)["rgb8"]}
            equal = True
            for k in (0, T // 3, T - 1):
                a = routes["bound"](k)
                torch.cuda.synchronize()
                a = a.clone()
                b = routes["unbound"](k)
                torch.cuda.synchronize()
                equal = equal and bool(torch.equal(a, b)) and int(a.max()) > 0
            cell = {"A": A, "frames_equal": equal, "bind_ms": round(bind_ms, 2)}
            meds = {r: [] for r in routes}
            for rep in range(args.reps):
                wall = timed_alternating(routes, args.steps, args.warmup if rep == 0 else 1, T)
                for r in routes:
                    meds[r].append(median(wall[r]))
            front = front_times(routes, args.steps, T)
            for r, fn in routes.items():
                cell[r] = dict(spread([round(x, 1) for x in meds[r]], prefix="wall_"), front_us=front[r],
                               host_syncs=count_syncs(lambda: fn(T // 2)))
            cell["unbound_minus_bound_us"] = round(cell["unbound"]["wall_us"] - cell["bound"]["wall_us"], 1)
            cell["spread_us"] = round(max(cell[r]["wall_max_us"] - cell[r]["wall_min_us"] for r in routes), 1)
            result["cases"]["A%d_%s" % (A, case)] = cell
            del session, sc
        del models, actors
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
