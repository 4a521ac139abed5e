"""The reference's mono-normal term (train.py:206-225 behind F.normalize, street_gaussian_renderer.py:245-246), its
scale-flatten and opacity-sparse regularisers (train.py:190-204, gaussian_model.py:271-280, the get_opacity
concatenation included) and its PSNR (loss_utils.py:61-78) as PyTorch code against the fused HIP paths
(gaussianrpg_amd.loss.normal_loss / scale_flatten_loss / opacity_sparse_loss / gaussian_reg_loss / psnr) on the same
device: the normal term and PSNR at 1920x1280, the regularisers at P = 1 M in one model and at 1.9 M + 10 x 10 k in
eleven models.  Forward + backward (PSNR: forward only).  Each entry holds forward ms, backward ms and ms for both: the
median of --rounds x --steps timed iterations (device events around work that ends in a synchronise, after --warmup),
the two paths alternating round by round so that both see the same machine.  For the fused path also the bytes the
algorithm needs per call and the achieved GB/s over the event time; the event times include
the launches and the tiny reduce kernel, so the kernel-only rate is higher.  Prints one JSON line; --out writes it
to a file as well."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from benchkit import median
from gaussianrpg_amd import loss as fused_loss

HBM_PEAK_GBS = 8000.0


# ---- the reference's expressions ----

def torch_normal(normals, mono, wvt, mask, sky):
    normals = torch.nn.functional.normalize(normals, dim=0)
    normal_mask = torch.logical_and(mask, ~sky)
    normal_mask = normal_mask.squeeze(0)
    normal_mask[:50] = False
    normal_gt = mono.permute(1, 2, 0)
    R_c2w = wvt[:3, :3]
    normal_gt = torch.matmul(normal_gt, R_c2w.T)
    normal_pred = normals.permute(1, 2, 0)
    normal_l1_loss = torch.abs(normal_pred[normal_mask] - normal_gt[normal_mask]).mean()
    normal_cos_loss = (1. - torch.sum(normal_pred[normal_mask] * normal_gt[normal_mask], dim=-1)).mean()
    return normal_l1_loss + normal_cos_loss


def torch_scale_flatten(scaling):
    scales = torch.exp(scaling)
    sorted_scales = torch.sort(scales, dim=1, descending=False).values
    s1, s2, s3 = sorted_scales[:, 0], sorted_scales[:, 1], sorted_scales[:, 2]
    s1 = torch.clamp(s1, 0, 30)
    s2 = torch.clamp(s2, 1e-5, 30)
    s3 = torch.clamp(s3, 1e-5, 30)
    return torch.abs(s1).mean() + torch.abs(s2 / s3 + s3 / s2 - 2.).mean()


def torch_opacity_sparse(opacities, radii):
    opacity = torch.cat([torch.sigmoid(o) for o in opacities], dim=0)      # get_opacity
    visibility_filter = radii > 0
    opacity = opacity.clamp(1e-6, 1 - 1e-6)
    log_opacity = opacity * torch.log(opacity)
    log_one_minus_opacity = (1 - opacity) * torch.log(1 - opacity)
    return -1 * (log_opacity + log_one_minus_opacity)[visibility_filter].mean()


def torch_psnr(img1, img2, mask):
    img1 = img1.permute(1, 2, 0)
    img2 = img2.permute(1, 2, 0)
    mask = mask.squeeze(0)
    img1 = img1[mask]
    img2 = img2[mask]
    mse = torch.mean((img1 - img2) ** 2)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


# ---- timing ----

class Timed:
    """One path of one row: fn(*leaves) -> loss; the leaves receive gradients (none: forward only)."""

    def __init__(self, fn, leaves):
        self.fn, self.leaves = fn, leaves
        self.fw, self.bw, self.both = [], [], []

    def run(self, steps, record):
        for _ in range(steps):
            for x in self.leaves:
                x.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            e[0].record()
            v = self.fn(*self.leaves)
            e[1].record()
            if self.leaves:
                v.backward()
            e[2].record()
            torch.cuda.synchronize()
            if record:
                self.fw.append(e[0].elapsed_time(e[1]))
                self.bw.append(e[1].elapsed_time(e[2]))
                self.both.append(e[0].elapsed_time(e[2]))

    def result(self):
        r = {"forward_ms": median(self.fw)}
        if self.leaves:
            r["backward_ms"], r["fwd_bwd_ms"] = median(self.bw), median(self.both)
        return r


def compare(out, name, torch_path, fused_path, args, fwd_bytes, bwd_bytes=None):
    for p in (torch_path, fused_path):
        p.run(args.warmup, False)
    for _ in range(args.rounds):                      # alternate: both paths see the same machine
        torch_path.run(args.steps, True)
        fused_path.run(args.steps, True)
    t, f = torch_path.result(), fused_path.result()
    f["forward_bytes"] = fwd_bytes
    f["forward_gbs"] = fwd_bytes / f["forward_ms"] * 1e-6
    f["forward_share_of_8tbs"] = f["forward_gbs"] / HBM_PEAK_GBS
    if bwd_bytes is not None:
        f["backward_bytes"] = bwd_bytes
        f["backward_gbs"] = bwd_bytes / f["backward_ms"] * 1e-6
        f["backward_share_of_8tbs"] = f["backward_gbs"] / HBM_PEAK_GBS
    key = "fwd_bwd_ms" if bwd_bytes is not None else "forward_ms"
    out[name + "_torch"], out[name + "_fused"] = t, f
    out[name + "_speedup"] = t[key] / f[key]


def _leaf(t):
    return t.clone().requires_grad_(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--background", type=int, default=1_900_000)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--object-points", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    benchkit.require_gpu("bench_reg_losses")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    n = H * W
    g = torch.Generator().manual_seed(H + W)
    out = {"bench": "tools/bench_reg_losses.py: train.py normal / scale-flatten / opacity-sparse terms fwd + bwd and "
                    "PSNR, %dx%d, P = %d and %d + %d x %d" % (W, H, args.points, args.background, args.objects,
                                                             args.object_points),
           "steps": args.steps, "rounds": args.rounds}

    # the mono-normal term: 80 % mask, 30 % sky, the first 50 rows off
    normals = (torch.randn(3, H, W, generator=g) * 0.7).to(dev)
    mono = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0).to(dev)
    wvt = torch.eye(4)
    wvt[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    wvt = wvt.to(dev)
    mask = (torch.rand(1, H, W, generator=g) < 0.8).to(dev)
    sky = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    nsel = int(((mask & ~sky)[0, 50:]).sum())
    compare(out, "normal", Timed(lambda x: torch_normal(x, mono, wvt, mask, sky), [_leaf(normals)]),
            Timed(lambda x: fused_loss.normal_loss(x, mono, wvt, mask, sky), [_leaf(normals)]), args,
            2 * n + 24 * nsel, 2 * n + 12 * n + 24 * nsel)

    # PSNR with the training mask
    img = torch.rand(3, H, W, generator=g).to(dev)
    gt = (img.cpu() + torch.randn(3, H, W, generator=g) * 0.05).clamp(0, 1).to(dev)
    compare(out, "psnr", Timed(lambda: torch_psnr(img, gt, mask), []), Timed(lambda: fused_loss.psnr(img, gt, mask), []),
            args, n + 24 * int(mask.sum()))

    # the regularisers: one model of P, and a background of 1.9 M with ten objects of 10 k
    for name, sizes in (("P%d" % args.points, [args.points]),
                        ("models%d" % (args.objects + 1), [args.background] + [args.object_points] * args.objects)):
        P = sum(sizes)
        scaling = (torch.randn(sizes[0], 3, generator=g) * 1.5 - 3).to(dev)          # the background model's
        opacities = [(torch.randn(s, 1, generator=g) * 4).to(dev) for s in sizes]
        radii = ((torch.rand(P, generator=g) < 0.6).int() * 7).to(dev)
        nvis = int((radii > 0).sum())
        compare(out, "scale_flatten_" + name, Timed(torch_scale_flatten, [_leaf(scaling)]),
                Timed(fused_loss.scale_flatten_loss, [_leaf(scaling)]), args, 12 * sizes[0], 24 * sizes[0])
        compare(out, "opacity_sparse_" + name,
                Timed(lambda *o: torch_opacity_sparse(o, radii), [_leaf(o) for o in opacities]),
                Timed(lambda *o: fused_loss.opacity_sparse_loss(list(o), radii), [_leaf(o) for o in opacities]), args,
                4 * P + 4 * nvis, 8 * P + 4 * nvis)
        compare(out, "both_" + name,
                Timed(lambda s, *o: 0.1 * torch_scale_flatten(s) + 0.1 * torch_opacity_sparse(o, radii),
                      [_leaf(scaling)] + [_leaf(o) for o in opacities]),
                Timed(lambda s, *o: fused_loss.gaussian_reg_loss(scaling=s, opacities=list(o), radii=radii,
                                                                 lambda_scale_flatten=0.1, lambda_opacity_sparse=0.1)[0],
                      [_leaf(scaling)] + [_leaf(o) for o in opacities]), args,
                12 * sizes[0] + 4 * P + 4 * nvis, 24 * sizes[0] + 8 * P + 4 * nvis)
    benchkit.emit(out, args.out)


if __name__ == "__main__":
    main()
