"""The reference's auxiliary training terms (train.py:121-127 sky, 145-158 obj_acc_loss, 164-176 lidar depth) as
PyTorch code against the fused HIP path (gaussianrpg_amd.loss.aux_loss), forward + backward: at 1920x1280 and
1242x375, lidar coverage 5 % (sparse, like projected Waymo sweeps) and 66 % (bench.py's synthetic density), with and
without the object term.  Each entry holds forward ms, backward ms and ms for both, the median of --steps timed
iterations (CUDA events, after --warmup).  Also the config-5 training step (P = 1 M street scene at 1920x1280: the
op's forward, the fused L1 + SSIM mix, the aux terms, the backward of all), with no aux terms, with the PyTorch ones
and with the fused ones.  Prints one JSON line."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from benchkit import median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import loss as fused_loss

LAMBDA_LIDAR, LAMBDA_SKY, LAMBDA_REG = 0.1, 0.05, 0.1


def torch_aux(depth, acc, lidar, mask, sky, acc_obj, bound):
    """train.py's code for the three terms, in its order (sky, obj, lidar)."""
    a = torch.clamp(acc, min=1e-6, max=1. - 1e-6)
    loss = LAMBDA_SKY * torch.where(sky, -torch.log(1 - a), -torch.log(a)).mean()
    if acc_obj is not None:
        ao = torch.clamp(acc_obj, min=1e-6, max=1. - 1e-6)
        loss = loss + LAMBDA_REG * torch.where(bound, -(ao * torch.log(ao) + (1. - ao) * torch.log(1. - ao)),
                                               -torch.log(1. - ao)).mean()
    depth_mask = torch.logical_and(lidar > 0., mask)
    if torch.nonzero(depth_mask).any():
        expected = depth / (acc + 1e-10)
        err = torch.abs(expected[depth_mask] - lidar[depth_mask])
        err, _ = torch.topk(err, int(0.95 * err.size(0)), largest=False)
        loss = loss + LAMBDA_LIDAR * err.mean()
    return loss


def fused_aux(depth, acc, lidar, mask, sky, acc_obj, bound):
    return fused_loss.aux_loss(depth, acc, lidar_depth=lidar, mask=mask, sky_mask=sky, acc_obj=acc_obj,
                               obj_bound=bound, lambda_depth_lidar=LAMBDA_LIDAR, lambda_sky=LAMBDA_SKY,
                               lambda_reg=LAMBDA_REG)[0]


def _planes(H, W, coverage, dev):
    g = torch.Generator().manual_seed(H + W)
    depth = (torch.rand(1, H, W, generator=g) * 60 + 1).to(dev)
    acc = torch.rand(1, H, W, generator=g).to(dev)
    lidar = torch.rand(1, H, W, generator=g) * 80
    lidar[torch.rand(1, H, W, generator=g) >= coverage] = 0
    mask = (torch.rand(1, H, W, generator=g) > 0.05).to(dev)
    sky = (torch.rand(1, H, W, generator=g) < 0.25).to(dev)
    acc_obj = torch.rand(1, H, W, generator=g).to(dev)
    bound = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    return depth, acc, lidar.to(dev), mask, sky, acc_obj, bound


def time_loss(fn, planes, with_obj, steps, warmup):
    depth, acc, lidar, mask, sky, acc_obj, bound = planes
    fw, bw, both = [], [], []
    for it in range(warmup + steps):
        d, a = depth.clone().requires_grad_(True), acc.clone().requires_grad_(True)
        ao = acc_obj.clone().requires_grad_(True) if with_obj else None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        l = fn(d, a, lidar, mask, sky, ao, bound)
        e[1].record()
        l.backward()
        e[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            both.append(e[0].elapsed_time(e[2]))
    return {"forward_ms": median(fw), "backward_ms": median(bw), "fwd_bwd_ms": median(both)}


def time_train_step(aux_fn, P, steps, warmup, dev):
    sc = hz.street_scene(P, seed=149).to(dev)
    leaves = hz.Scene(*(t.clone().requires_grad_(True) if isinstance(t, torch.Tensor) else t for t in sc))
    H, W = hz.WAYMO_H, hz.WAYMO_W
    gt = torch.rand(3, H, W, device=dev)
    _, _, lidar, mask, sky, _, bound = _planes(H, W, 0.66, dev)
    frames = iter(range(warmup + steps))

    def prepare():
        for t in leaves:
            if isinstance(t, torch.Tensor):
                t.grad = None
        return hz.trajectory_camera(next(frames) % 200, device=dev)

    def step(cam):
        pkg = hz.render_kernel(leaves, cam, mode="train")
        loss = fused_loss.l1_ssim_loss(pkg["rgb"], gt, lambda_l1=1.0, lambda_dssim=0.2)[0]
        # acc stands in for the object render's acc_obj (the second render is not part of this measurement)
        if aux_fn is not None:
            loss = loss + aux_fn(pkg["depth"], pkg["acc"], lidar, mask, sky, pkg["acc"], bound)
        loss.backward()
        return pkg, loss    # held until after the synchronize, as before
    return benchkit.medians(benchkit.timed(step, steps, warmup, prepare=prepare, wall=False))["device_us"] / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--no-train-step", action="store_true")
    args = ap.parse_args()
    benchkit.require_gpu("bench_aux_loss")
    dev = torch.device("cuda:0")
    out = {"bench": "tools/bench_aux_loss.py: train.py lidar (0.1), sky (0.05), obj (0.1) terms, fwd + bwd",
           "steps": args.steps}
    for W, H in ((1920, 1280), (1242, 375)):
        for cov in (0.05, 0.66):
            planes = _planes(H, W, cov, dev)
            for with_obj in (False, True):
                for name, fn in (("torch", torch_aux), ("fused", fused_aux)):
                    key = "%dx%d_cov%02d_%s_%s" % (W, H, round(100 * cov), "obj" if with_obj else "noobj", name)
                    out[key] = time_loss(fn, planes, with_obj, args.steps, args.warmup)
    if not args.no_train_step:
        for name, fn in (("none", None), ("torch", torch_aux), ("fused", fused_aux)):
            out["train_step_P%d_1920x1280_aux_%s_ms" % (args.gaussians, name)] = time_train_step(
                fn, args.gaussians, max(args.steps // 3, 5), args.warmup, dev)
    benchkit.emit(out)


if __name__ == "__main__":
    main()
