"""Pose correction of the background (gaussianrpg_amd/pose_correction.py, csrc/pose_correction.hip), routes timed on the
same GPU in ONE process, alternating batch by batch:
(a) the op alone at N = 1 M and 1.9 M rows: ``pose_correct(xyz, rotation, rot, trans)`` against the reference's lines in
    PyTorch on the device (``harness.pose_correct_torch``: camera_pose.py:89-114), forward and forward + backward to
    xyz, rotation and the row; the forward's byte floor (28 B read and 28 B written per row at 8 TB/s) and the fraction
    of it reached;
(b) the training step (forward + backward, ``harness.corrected_train_step``) at 1.9 M background Gaussians + 10 actors of
    10 k (``harness.actor_scene``), 1920x1280: ``ComposedRasterizer`` with the background's device row
    (``PoseCorrection.rows``) against the SAME step uncorrected (``active=False``: the background static), against the
    reference's composition in PyTorch with ``pose_correct`` and the classic op, and against that with the correction
    in PyTorch as well;
(c) the evaluation frame (``harness.corrected_frame``), likewise.
Per route: the device time per call between two events around a batch of --inner back-to-back calls and the wall time
per call between two synchronises; median over --batches batches after --warmup batches, --reps times; per cell the
median of the repetitions and all of them (their spread).  For the composed routes of (b) and (c) also the device
kernels of one call with their times (torch.profiler; null where it is not available), so that a difference between
the corrected and the uncorrected step can be laid at a kernel's door.  No speed threshold belongs to this tool.
Prints one JSON line; --out FILE also writes it (profiles/pose_correction_bench.json)."""
import argparse, os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import benchkit
from benchkit import column, median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import ModelParams
from gaussianrpg_amd.pose_correction import PoseCorrection, pose_correct
from gaussianrpg_amd.rasterizer import GaussianRasterizationSettings
from gaussianrpg_amd.tracks import PoseBatch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=20, help="back-to-back calls of the op per batch")
ap.add_argument("--inner-step", type=int, default=4, help="back-to-back training steps / frames per batch")
ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 1_900_000])
ap.add_argument("--background", type=int, default=1_900_000)
ap.add_argument("--actors", type=int, default=10)
ap.add_argument("--actor-size", type=int, default=10_000)
ap.add_argument("--only", choices=["op", "step", "frame"], action="append")
args = ap.parse_args()
only = args.only or ["op", "step", "frame"]

benchkit.require_gpu("bench_pose_correction")
dev = torch.device("cuda:0")
PEAK_BYTES_PER_S = 8e12


def alternate(routes, inner):
    reps = {k: {"wall": [], "device": []} for k in routes}
    for _ in range(args.reps):
        seen = benchkit.alternating(routes, args.batches, args.warmup, inner=inner)
        for k in routes:
            reps[k]["wall"].append(median(column(seen[k], "wall_us")))
            reps[k]["device"].append(median(column(seen[k], "device_us")))
    return {k: {"wall_us": median(reps[k]["wall"]), "wall_repetitions_us": reps[k]["wall"],
                "device_us": median(reps[k]["device"]), "device_repetitions_us": reps[k]["device"],
                "device_spread_us": max(reps[k]["device"]) - min(reps[k]["device"])} for k in routes}


def kernels(fn):
    """[(kernel, calls, total us)] of one call, longest first, or an error record where the profiler cannot tell."""
    def figure():
        fn()
        agg = {}
        for name, us in benchkit.device_kernels(fn):
            c = agg.setdefault(name[:96], [0, 0.0])
            c[0] += 1
            c[1] += us
        return [dict(kernel=k, calls=v[0], us=v[1]) for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])][:24] or None
    return benchkit.optional(figure)


result = {"what": "pose correction of the background; us per call: per cell the median over %d repetitions of (median "
                  "over %d batches of back-to-back calls between two device events / two synchronises, after %d "
                  "warm-up batches); the routes alternate batch by batch in one process"
                  % (args.reps, args.batches, args.warmup),
          "device": torch.cuda.get_device_name(0), "op": {}, "step": {}, "frame": {}}
g = torch.Generator().manual_seed(17)
row_rot = (torch.tensor([1.0, 0.0, 0.0, 0.0]) + 0.01 * (torch.rand(4, generator=g) - 0.5)).to(dev).requires_grad_(True)
row_trans = (0.05 * (torch.rand(3, generator=g) - 0.5)).to(dev).requires_grad_(True)

# ---- (a) the op alone ----
if "op" in only:
    for N in args.sizes:
        xyz = ((torch.rand(N, 3, generator=g) - 0.5) * 120.0).to(dev).requires_grad_(True)
        rotation = torch.nn.functional.normalize(torch.randn(N, 4, generator=g)).to(dev).requires_grad_(True)
        up_x, up_r = torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 4, generator=g).to(dev)
        leaves = (xyz, rotation, row_rot, row_trans)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(xyz, rotation, row_rot, row_trans)
            return run

        def fwd_bwd(fn):
            def run():
                ox, orot = fn(xyz, rotation, row_rot, row_trans)
                return torch.autograd.grad((ox, orot), leaves, (up_x, up_r))
            return run

        cell = {"forward": alternate({"fused": fwd(pose_correct), "torch": fwd(hz.pose_correct_torch)}, args.inner),
                "forward_backward": alternate({"fused": fwd_bwd(pose_correct), "torch": fwd_bwd(hz.pose_correct_torch)},
                                              args.inner)}
        floor_us = N * 56 / PEAK_BYTES_PER_S * 1e6
        cell["forward_byte_floor_us"] = floor_us
        cell["forward_fraction_of_floor"] = floor_us / cell["forward"]["fused"]["device_us"]
        for k in ("forward", "forward_backward"):
            cell[k]["torch_over_fused_device"] = cell[k]["torch"]["device_us"] / cell[k]["fused"]["device_us"]
        result["op"][str(N)] = cell
        del xyz, rotation, up_x, up_r, leaves
        torch.cuda.empty_cache()

# ---- (b), (c): the scene of tools/bench_compose.py as harness.actor_scene builds it ----
if "step" in only or "frame" in only:
    NB, NA, PA = args.background, args.actors, args.actor_size
    sc, _ = hz.actor_scene(NB, NA, PA)

    def raw(lo, hi):
        op = sc.opacity[lo:hi].clamp(1e-4, 1 - 1e-4)
        return ModelParams(*(t.contiguous().to(dev).requires_grad_(True) for t in (
            sc.means3D[lo:hi], torch.log(sc.scales[lo:hi]), sc.rotations[lo:hi] * 1.7, torch.log(op / (1 - op)),
            sc.shs[lo:hi, :1], sc.shs[lo:hi, 1:])))

    models = [raw(0, NB)] + [raw(NB + k * PA, NB + (k + 1) * PA) for k in range(NA)]
    del sc
    # the actors' Gaussians are in world coordinates already: a pose next to the identity keeps them on the road
    a_rot = torch.nn.functional.normalize(torch.tensor([[1.0, 0.0, 0.01 * (k + 1), 0.0] for k in range(NA)]))
    a_trans = torch.tensor([[0.01 * k, 0.0, 0.02 * k] for k in range(NA)])
    batch_poses = PoseBatch(a_rot.unsqueeze(0).to(dev).requires_grad_(True), a_trans.unsqueeze(0).to(dev).requires_grad_(True),
                            torch.ones(1, NA, dtype=torch.uint8, device=dev))
    visible, times = list(range(NA)), [0.0] * NA
    cam = hz.trajectory_camera(0, device=dev)
    settings = GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))
    camera = types.SimpleNamespace(id=1, meta=dict(frame_idx=1))
    pc = PoseCorrection(4).to(dev)
    with torch.no_grad():
        pc.pose_correction_rots[1] = row_rot.detach()
        pc.pose_correction_trans[1] = row_trans.detach()
    off = PoseCorrection(4, active=False).to(dev)
    P = NB + NA * PA
    params = [t for m in models for t in m[:6]] + [batch_poses.rot, batch_poses.trans] + list(pc.parameters())

    def zero():
        for t in params:
            t.grad = None

    def step(module, **kw):
        def run():
            zero()
            m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
            hz.corrected_train_step(settings, models, batch_poses, 0, visible, times, module, camera, means2D=m2d, **kw)
        return run

    def frame(module, **kw):
        def run():
            return hz.corrected_frame(settings, models, batch_poses, 0, visible, times, module, camera, **kw)
        return run

    for name, make in (("step", step), ("frame", frame)):
        if name not in only:
            continue
        routes = {"composed_corrected": make(pc, composed=True), "composed_uncorrected": make(off, composed=True),
                  "classic_pose_correct": make(pc, composed=False, fused=True),
                  "classic_torch": make(pc, composed=False, fused=False)}
        cell = alternate(routes, args.inner_step)
        parent = cell["composed_uncorrected"]
        cell["corrected_minus_uncorrected_device_us"] = cell["composed_corrected"]["device_us"] - parent["device_us"]
        cell["uncorrected_spread_device_us"] = parent["device_spread_us"]
        cell["classic_pose_correct_over_composed_device"] = \
            cell["classic_pose_correct"]["device_us"] / cell["composed_corrected"]["device_us"]
        cell["classic_torch_over_classic_pose_correct_device"] = \
            cell["classic_torch"]["device_us"] / cell["classic_pose_correct"]["device_us"]
        cell["kernels"] = {k: kernels(routes[k]) for k in ("composed_corrected", "composed_uncorrected")}
        result[name] = cell
        result[name]["scene"] = "%d background + %d x %d, %dx%d" % (NB, NA, PA, int(cam.image_width), int(cam.image_height))

benchkit.emit(result, args.out)
