"""Hashes of the fused losses' values and input gradients on fixed, seeded inputs (public gaussianrpg_amd.loss API
only), for bit-for-bit comparisons of two builds on one box: run it from each build's own checkout and compare the
printed lines."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gaussianrpg_amd import loss
dev = torch.device("cuda:0")
def h(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:12]
def leaf(t):
    return t.to(dev).requires_grad_(True)
for H, W in ((37, 53), (1280, 1920)):
    g = torch.Generator().manual_seed(H + W)
    a = torch.rand(3, H, W, generator=g)
    gt = (a + 0.2 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
    m = (torch.rand(1, H, W, generator=g) > 0.3).to(dev)
    x = leaf(a)
    l, l1, ss = loss.l1_ssim_loss(x, gt, m)
    l.backward()
    print("l1_ssim %dx%d" % (H, W), "loss", h(l), "l1", h(l1), "ssim", h(ss), "grad", h(x.grad))
    acc, acc_obj = torch.rand(H, W, generator=g), torch.rand(H, W, generator=g)
    lidar = torch.where(torch.rand(H, W, generator=g) < 0.3, 5 + 40 * torch.rand(H, W, generator=g), torch.zeros(H, W))
    depth = acc * (lidar + 2 * torch.randn(H, W, generator=g)).abs()
    mask, sky, bound = ((torch.rand(H, W, generator=g) > p).to(dev) for p in (0.1, 0.7, 0.5))
    lidar = lidar.to(dev)
    d, ac, ao = leaf(depth), leaf(acc), leaf(acc_obj)
    l, terms = loss.aux_loss(d, ac, lidar_depth=lidar, mask=mask, sky_mask=sky, sky_scale=0.7, acc_obj=ao,
                             obj_bound=bound, lambda_depth_lidar=0.1, lambda_sky=0.05, lambda_reg=0.02)
    l.backward()
    print("aux %dx%d" % (H, W), "loss", h(l), *["%s %s" % (k, h(v)) for k, v in sorted(terms.items())],
          "grads", h(d.grad), h(ac.grad), h(ao.grad))
    sel = loss.lidar_selection(d.detach(), ac.detach(), lidar, mask)
    print("lidar_selection %dx%d" % (H, W), *["%s %s" % (k, h(v)) for k, v in sorted(sel.items())])
for S, H, W in ((19, 37, 53), (40, 96, 200)):
    g = torch.Generator().manual_seed(1000 * S + H)
    gt = torch.randint(0, S, (H, W), generator=g)
    gt[torch.rand(H, W, generator=g) < 0.2] = -1
    gt = gt.to(dev)
    for mode in ("logits", "probabilities"):
        sem = torch.randn(S, H, W, generator=g) if mode == "logits" else torch.rand(S, H, W, generator=g) * 0.98 + 0.01
        x = leaf(sem)
        l = loss.semantic_loss(x, gt, mode=mode)
        l.backward()
        st = loss.semantic_loss_stats(x.detach(), gt, mode=mode)
        print("semantic S=%d %dx%d %s" % (S, H, W, mode), "loss", h(l), "grad", h(x.grad),
              *["%s %s" % (k, h(v)) for k, v in sorted(st.items())])
