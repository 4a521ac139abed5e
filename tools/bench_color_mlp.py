"""Colour correction, use_mlp variant (gaussianrpg_amd/appearance.py ColorCorrectionMLP, csrc/color_mlp.hip): camera
pose -> the two 3x4 matrices, two routes timed on the same GPU in ONE process, alternating call by call:
(a) fused    ColorCorrectionMLP.affines_and_reg: one launch forward, one launch backward, no host wait;
(b) torch    harness.camera_affine(fused=False)'s computation: the 4x4 product, the axis-angle in ordinary PyTorch with
             boolean-mask indexing, the two nn.Sequential networks, + identity, the regulariser in PyTorch.
Cases: T = 1 evaluation (both matrices under no_grad); T = 1 training (both matrices and the regulariser, a weighted
sum as the loss, backward to the sixteen tensors); T = 200 evaluation (a trajectory's matrices in one call).  Also one
evaluation frame through harness.simulator_frame_corrected(one_call=True) with the module in place of the matrix
against the same frame fed the torch route's matrix.
Per route and case: wall time of one call on the host with the device idle before it and waited for after it, and the
time between two device events around it; median over --steps calls, --reps times, median of those with the spread.
Also the host synchronisations torch sees in one call (sync debug mode) and the device kernels one call launches
(torch.profiler; null where the profiler is not available).
No speed threshold belongs to this tool: the op is launch-sized, and the claim it measures is the launches and waits it
removes.  Prints one JSON line; --out FILE also writes it (profiles/color_mlp_bench.json)."""
import argparse
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import benchkit
from benchkit import count_syncs, median, spread
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.appearance import ColorCorrectionMLP


def poses(T, dev, seed=0):
    """T ego poses along a gently curving track (a few hundred metres) and one camera extrinsic."""
    rng = np.random.RandomState(seed)
    ego = np.tile(np.eye(4, dtype=np.float32), (T, 1, 1))
    yaw = 0.4 + 0.004 * np.arange(T) + rng.normal(0, 0.002, T)
    ego[:, 0, 0], ego[:, 0, 1], ego[:, 1, 0], ego[:, 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    ego[:, :3, 3] = np.stack([120.0 + 1.5 * np.arange(T), -80.0 + 0.2 * np.arange(T), np.full(T, 1.9)], 1)
    ext = np.eye(4, dtype=np.float32)
    ext[:3, :3] = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    ext[:3, 3] = (1.5, 0.0, 2.1)
    return torch.from_numpy(ego).to(dev), torch.from_numpy(ext).to(dev)[None]


def count_own_launches(fn):
    """benchkit.count_launches, plus how many of the kernels are this op's own (color_mlp_*): the rest of a training
    call is the loss arithmetic around it (products, sums and their autograd), the same on both routes."""
    def figure():
        kernels = benchkit.device_kernels(fn)
        out = benchkit.launch_counts(kernels)
        if out is not None:
            out["color_mlp_forward_kernels"] = sum("color_mlp_forward" in n for n, _ in kernels)
            out["color_mlp_backward_kernels"] = sum("color_mlp_backward" in n for n, _ in kernels)
        return out
    return benchkit.optional(figure)


def torch_route(cc, ego, ext, reg):
    x = hz._axis_angle_torch(ego @ ext)
    eye = cc.identity_matrix
    A = cc.affine_trans(x).view(-1, 3, 4) + eye
    S = cc.affine_trans_sky(x).view(-1, 3, 4) + eye
    out = torch.stack([A, S], 1)
    if not reg:
        return out, None
    return out, (torch.abs(A - eye) + torch.abs(S - eye)).mean((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=300000)
    args = ap.parse_args()
    benchkit.require_gpu("bench_color_mlp")
    dev = torch.device("cuda:0")
    result = {"bench": "tools/bench_color_mlp.py: pose -> colour-correction matrices of the use_mlp variant, fused HIP "
                       "against ordinary PyTorch; us per call (wall on the host with the device idle before and waited "
                       "for after, and between two device events), median over %d calls, median of %d repetitions; "
                       "the routes alternate in one process" % (args.steps, args.reps),
              "device": torch.cuda.get_device_name(0), "cases": {}}
    torch.manual_seed(0)
    cc = ColorCorrectionMLP().to(dev)
    with torch.no_grad():
        for net in (cc.affine_trans, cc.affine_trans_sky):      # a trained module: the last layer is not zero
            net[6].weight.normal_(0, 0.01)
            net[6].bias.normal_(0, 0.01)

    def case(name, T, train):
        ego, ext = poses(T, dev)
        ga, gr = torch.randn(T, 2, 3, 4, device=dev), torch.randn(T, device=dev)

        def run(fused):
            if not train:
                with torch.no_grad():
                    return (cc.affines(ego, ext),) if fused else (torch_route(cc, ego, ext.expand(T, 4, 4), False)[0],)
            cc.zero_grad(set_to_none=True)
            if fused:
                A, reg, _ = cc.affines_and_reg(ego, ext)
            else:
                A, reg = torch_route(cc, ego, ext.expand(T, 4, 4), True)
            ((A * ga).sum() + (reg * gr).sum()).backward()
            return (A.detach(),) + tuple(p.grad for p in cc.parameters())

        routes = {"fused": lambda: run(True), "torch": lambda: run(False)}
        a, b = run(True), [t.clone() for t in run(False)]
        cell = {"T": T, "max_abs_difference_between_routes": max(float((x - y).abs().max()) for x, y in zip(a, b))}
        reps = benchkit.windows(routes, args.reps, args.steps, args.warmup)
        for k, fn in routes.items():
            cell[k] = dict(spread(reps[k]["wall_us"], prefix="wall_"), device_events_us=median(reps[k]["device_us"]),
                           host_syncs=count_syncs(fn), launches=count_own_launches(fn))
        cell["torch_over_fused_wall"] = cell["torch"]["wall_us"] / cell["fused"]["wall_us"]
        result["cases"][name] = cell

    case("T1_evaluation", 1, False)
    case("T1_training_with_regulariser", 1, True)
    case("T200_evaluation", 200, False)

    # one evaluation frame with the module in place of the matrix
    scene = hz.street_scene(P=args.points).to(dev)
    cam = hz.trajectory_camera(1, device=dev)
    ego, ext = poses(1, dev)
    camera = types.SimpleNamespace(ego_pose=ego[0], extrinsic=ext[0])
    out = torch.empty((int(cam.image_height), int(cam.image_width), 3), dtype=torch.uint8).pin_memory()

    def frame(fused):
        if fused:
            return hz.simulator_frame_corrected(scene, cam, cc, camera=camera, one_call=True, out=out)
        with torch.no_grad():
            A = hz.camera_affine(cc, camera, fused=False)
        return hz.simulator_frame_corrected(scene, cam, A, one_call=True, out=out)

    routes = {"fused": lambda: frame(True), "torch": lambda: frame(False)}
    a, b = frame(True).copy(), frame(False).copy()
    cell = {"points": args.points, "width": int(cam.image_width), "height": int(cam.image_height),
            "bytes_that_differ_between_routes": int((a != b).sum())}
    reps = benchkit.windows(routes, args.reps, args.steps, args.warmup)
    for k, fn in routes.items():
        cell[k] = dict(spread(reps[k]["wall_us"], prefix="wall_"), host_syncs=count_syncs(fn))
    cell["torch_over_fused_wall"] = cell["torch"]["wall_us"] / cell["fused"]["wall_us"]
    result["cases"]["evaluation_frame"] = cell
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
