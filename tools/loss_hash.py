"""Hashes of the fused losses' values and input gradients, and of the other leaf ops' outputs (Adam + densify
statistics, distCUDA2, sky cube map), on fixed, seeded inputs (public Python API only), for bit-for-bit comparisons of
two builds on one box: run it from each build's own checkout and compare the printed lines."""
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
H, W = 37, 53
g = torch.Generator().manual_seed(16)
nrm, mono = torch.randn(3, H, W, generator=g), torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
wvt = torch.eye(4)
wvt[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
mask, sky = ((torch.rand(H, W, generator=g) > p).to(dev) for p in (0.2, 0.8))
for name, sk in (("no sky", None), ("sky", sky)):
    x = leaf(nrm)
    l = loss.normal_loss(x, mono.to(dev), wvt.to(dev), mask, sk, top_rows=5)
    l.backward()
    t = loss.normal_loss_terms(x.detach(), mono.to(dev), wvt.to(dev), mask, sk, top_rows=5)
    print("normal %dx%d %s" % (H, W, name), "loss", h(l), "grad", h(x.grad), *["%s %s" % (k, h(v)) for k, v in sorted(t.items())])
sc, ops = leaf(torch.randn(63, 3, generator=g)), [leaf(2 * torch.randn(n, 1, generator=g)) for n in (40, 23)]
radii = torch.randint(-1, 4, (63,), generator=g).int().to(dev)
l, terms = loss.gaussian_reg_loss(scaling=sc, opacities=ops, radii=radii, lambda_scale_flatten=0.3, lambda_opacity_sparse=0.2)
l.backward()
print("reg 63 = 40 + 23", "loss", h(l), *["%s %s" % (k, h(v)) for k, v in sorted(terms.items())],
      "grads", h(sc.grad), *[h(o.grad) for o in ops])
a, b = torch.rand(3, H, W, generator=g).to(dev), torch.rand(3, H, W, generator=g).to(dev)
print("psnr 3x%dx%d" % (H, W), "masked", h(loss.psnr(a, b, mask)), "all", h(loss.psnr(a, b)))
from gaussianrpg_amd.optim import FusedAdam, fused_adam_step, densification_stats_update
buf = torch.zeros(63 + 5, device=dev)
params = [torch.nn.Parameter(torch.randn(4097, generator=g).to(dev)),
          torch.nn.Parameter(buf[1:64].copy_(torch.randn(63, generator=g))),      # 4 bytes off: the scalar path
          torch.nn.Parameter(torch.randn(4096, generator=g).to(dev))]
opts = [FusedAdam([params[0], params[1]], lr=0.01), FusedAdam([params[2]], lr=0.002, eps=1e-15)]
for step in range(3):
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    fused_adam_step(opts)
print("adam 4097 63(+1) 4096", *[h(p) for p in params],
      *[h(o.state[p][k]) for o in opts for gr in o.param_groups for p in gr["params"] for k in ("exp_avg", "exp_avg_sq")])
vg, rd = torch.randn(63, 3, generator=g).to(dev), torch.randint(-1, 9, (63,), generator=g).int().to(dev)
acc_, den = ([torch.rand(n, c, generator=g).to(dev) for n in (40, 20)] for c in (2, 1))
mx = [5 * torch.rand(n, generator=g).to(dev) for n in (40, 20)]
densification_stats_update(vg, rd, [(0, 40), (43, 63)], acc_, den, mx)
print("densify 63: [0,40) [43,63)", *[h(t) for ts in (acc_, den, mx) for t in ts])
from simple_knn._C import distCUDA2
print("distCUDA2 1000", h(distCUDA2(torch.randn(1000, 3, generator=g).to(dev))))
from gaussianrpg_amd.sky import SkyCubeMap
K = torch.tensor([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]])
w2c = torch.eye(4)
w2c[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
skymap = SkyCubeMap(8).to(dev)
with torch.no_grad():
    skymap.sky_cube_map.copy_((torch.rand(6, 8, 8, 3, generator=g) * 1.3 - 0.15).to(dev))
ac, rgb = leaf(0.9 * torch.rand(1, H, W, generator=g)), leaf(torch.rand(3, H, W, generator=g))
out = skymap.composite(rgb, ac, K, w2c, train=True)
(out * torch.randn(3, H, W, generator=g).to(dev)).sum().backward()
gc = skymap.sky_cube_map.grad
# the cube-map gradient is summed by float atomics: its bits depend on the order, its support and rounded sum do not
print("sky res 8 %dx%d" % (H, W), "lookup", h(skymap(K, w2c, H, W, ac.detach())), "composite", h(out),
      "eval", h(skymap.composite(rgb.detach(), ac.detach(), K, w2c, train=False)), "grads", h(rgb.grad), h(ac.grad),
      "cube texels %d sum %.5g" % (int((gc != 0).sum()), float(gc.double().sum())))
