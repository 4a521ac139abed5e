"""The reference's training loss (lib/utils/loss_utils.py + train.py:116-118, lambda_dssim 0.2) as PyTorch code
against the fused HIP path (gaussianrpg_amd.loss.l1_ssim_loss), at 1920x1280 and 1242x375, C = 3:
forward ms, backward ms and ms for both, each the median of --steps timed iterations (CUDA events, after
--warmup).  'torch' follows the reference's structure: the window built on the host and copied to the
device per call, five depthwise F.conv2d calls and the elementwise map, the L1 as a boolean-mask gather
when a mask is given.  Also the config-5 training step (P = 1 M street scene at 1920x1280, the op's forward
+ loss forward + loss backward + the op's backward) with this loss mix, both ways.
Prints one JSON line."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import benchkit
from benchkit import median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd import loss as fused_loss


def _window(channel):
    g = torch.tensor([math.exp(-((k - 5) ** 2) / 4.5) for k in range(11)])
    g = g / g.sum()
    return (g[:, None] @ g[None, :]).expand(channel, 1, 11, 11).contiguous()


def torch_ssim(img1, img2, mask=None):
    C = img1.size(-3)
    w = _window(C)
    if mask is not None:
        img1 = torch.where(mask, img1, torch.zeros_like(img1))
        img2 = torch.where(mask, img2, torch.zeros_like(img2))
    w = w.to(img1.device).type_as(img1)
    mu1 = F.conv2d(img1, w, padding=5, groups=C)
    mu2 = F.conv2d(img2, w, padding=5, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, w, padding=5, groups=C) - mu1_sq
    s2 = F.conv2d(img2 * img2, w, padding=5, groups=C) - mu2_sq
    s12 = F.conv2d(img1 * img2, w, padding=5, groups=C) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean()


def torch_l1(img, gt, mask=None):
    img, gt = img.permute(1, 2, 0), gt.permute(1, 2, 0)
    if mask is not None:
        m = mask.squeeze(0)
        img, gt = img[m], gt[m]
    return torch.abs(img - gt).mean()


def torch_mix(img, gt, mask=None, lam=0.2):
    return (1.0 - lam) * 1.0 * torch_l1(img, gt, mask) + lam * (1.0 - torch_ssim(img, gt, mask=mask))


def fused_mix(img, gt, mask=None, lam=0.2):
    return fused_loss.l1_ssim_loss(img, gt, mask, lambda_l1=1.0, lambda_dssim=lam)[0]


def time_loss(fn, H, W, mask, steps, warmup, dev):
    img = torch.rand(3, H, W, device=dev)
    gt = torch.rand(3, H, W, device=dev)
    fw, bw, both = [], [], []
    for it in range(warmup + steps):
        x = img.clone().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        l = fn(x, gt, mask)
        e[1].record()
        l.backward()
        e[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            both.append(e[0].elapsed_time(e[2]))
    return {"forward_ms": median(fw), "backward_ms": median(bw), "fwd_bwd_ms": median(both)}


def time_train_step(fn, P, steps, warmup, dev):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sc = hz.street_scene(P, seed=149).to(dev)
    leaves = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.opacity, sc.shs, sc.scales, sc.rotations)]
    gt = torch.rand(3, hz.WAYMO_H, hz.WAYMO_W, device=dev)
    frames = iter(range(warmup + steps))

    def prepare():
        cam = hz.trajectory_camera(next(frames) % 200, device=dev)
        for t in leaves:
            t.grad = None
        return (GaussianRasterizer(GaussianRasterizationSettings(**hz.settings_kwargs(cam, 1))),
                torch.zeros(P, 3, device=dev, requires_grad=True))

    def step(arg):
        rast, means2D = arg
        color = rast(means3D=leaves[0], means2D=means2D, opacities=leaves[1], shs=leaves[2], scales=leaves[3],
                     rotations=leaves[4])[0]
        fn(color, gt, None).backward()
        return color        # held until after the synchronize, as before
    return benchkit.medians(benchkit.timed(step, steps, warmup, prepare=prepare, wall=False))["device_us"] / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--no-train-step", action="store_true")
    args = ap.parse_args()
    benchkit.require_gpu("bench_ssim")
    dev = torch.device("cuda:0")
    out = {"bench": "tools/bench_ssim.py: train.py:118 loss mix (lambda_dssim 0.2), C=3", "steps": args.steps}
    for W, H in ((1920, 1280), (1242, 375)):
        mask = torch.rand(1, H, W, device=dev) > 0.1
        for mname, m in (("nomask", None), ("mask", mask)):
            for name, fn in (("torch", torch_mix), ("fused", fused_mix)):
                out["%dx%d_%s_%s" % (W, H, mname, name)] = time_loss(fn, H, W, m, args.steps, args.warmup, dev)
    if not args.no_train_step:
        for name, fn in (("torch", torch_mix), ("fused", fused_mix)):
            out["train_step_P%d_1920x1280_%s_ms" % (args.gaussians, name)] = time_train_step(
                fn, args.gaussians, max(args.steps // 3, 5), args.warmup, dev)
    benchkit.emit(out)


if __name__ == "__main__":
    main()
