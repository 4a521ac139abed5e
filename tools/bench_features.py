"""Training step (forward + backward down to the raw parameters) of a composed frame WITH feature planes:
(a) the path a user has without forward_features -- PyTorch composition (street_gaussian_model.py:296-453) with
    autograd, torch.cat of the semantic arrays (+ PyTorch normals), the classic op with semantics=;
(b) ComposedRasterizer.forward_features (grpg_forward_composed_features / grpg_backward_composed_features).
Scene: config 5's P = 1 M background + 10 actors x 10 k, 1920x1280, S = 15; run once more with the normals on
(F = 18).  Method of DESIGN.md section 13: two device synchronisations around each call, median of 30 calls, five
repetitions.  Prints one JSON line; --out FILE also writes it (profiles/features_bench.json).
--only fused|torch, --normals 0|1 and --reps N cut a run down to one cell (for a kernel trace of its own)."""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import benchkit
from benchkit import median
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.composed import ActorPose, ComposedRasterizer, ModelParams, idft_weights
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--only", choices=("fused", "torch"), default=None)
ap.add_argument("--normals", type=int, choices=(0, 1), default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--calls", type=int, default=30)
args = ap.parse_args()

benchkit.require_gpu("bench_features")
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(2)
NB, NA, PA, FD, S = 1_000_000, 10, 10_000, 5, 15
sc = hz.street_scene(NB, seed=149)
logit = lambda p: torch.log(p / (1 - p))   # noqa: E731
models = [ModelParams(sc.means3D, torch.log(sc.scales), sc.rotations * 1.7, logit(sc.opacity.clamp(1e-4, 1 - 1e-4)),
                      sc.shs[:, :1].contiguous(), sc.shs[:, 1:].contiguous())]
for k in range(NA):
    models.append(ModelParams((torch.rand(PA, 3, generator=g) - 0.5) * torch.tensor([4.5, 1.6, 2.0]),
                              math.log(0.05) + 0.5 * torch.randn(PA, 3, generator=g),
                              torch.randn(PA, 4, generator=g), 1.0 + 2.0 * torch.randn(PA, 1, generator=g),
                              0.5 * torch.randn(PA, FD, 3, generator=g), 0.15 * torch.randn(PA, 3, 3, generator=g)))
models = [ModelParams(*(t.to(dev).requires_grad_(True) for t in m[:6])) for m in models]
sems = [torch.randn(m.xyz.shape[0], S, generator=g).to(dev).requires_grad_(True) for m in models]
P = sum(m.xyz.shape[0] for m in models)


def poses_at(f):
    out = [None]
    for k in range(NA):
        a = 0.05 * k + 0.002 * f
        out.append(ActorPose([math.cos(a), 0.0, math.sin(a), 0.0], [-12.0 + 2.5 * k, 0.8, 10.0 + 8.0 * k + 0.5 * f],
                             0.1 + 0.004 * f))
    return out


def qmul(a, b):
    aw, ax, ay, az = torch.unbind(a, -1); bw, bx, by, bz = torch.unbind(b, -1)
    return torch.stack((aw*bw-ax*bx-ay*by-az*bz, aw*bx+ax*bw+ay*bz-az*by, aw*by-ax*bz+ay*bw+az*bx,
                        aw*bz+ax*by-ay*bx+az*bw), -1)


def qmat(r):
    q = r / torch.sqrt((r * r).sum(1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1-2*(y*y+z*z), 2*(x*y-w*z), 2*(x*z+w*y), 2*(x*y+w*z), 1-2*(x*x+z*z), 2*(y*z-w*x),
                        2*(x*z-w*y), 2*(y*z+w*x), 1-2*(x*x+y*y)], 1).reshape(-1, 3, 3)


def torch_compose(poses):
    """the reference's getters (street_gaussian_model.py:296-453) on the device, with autograd"""
    xyz, sca, rot, opa, fea = [models[0].xyz], [torch.exp(models[0].scaling)], \
        [torch.nn.functional.normalize(models[0].rotation)], [torch.sigmoid(models[0].opacity)], \
        [torch.cat((models[0].features_dc, models[0].features_rest), 1)]
    loc_x = torch.cat([m.xyz for m in models[1:]])
    loc_r = torch.cat([torch.nn.functional.normalize(m.rotation) for m in models[1:]])
    orot = torch.cat([torch.tensor(p.obj_rot, device=dev).expand(PA, -1) for p in poses[1:]])
    otr = torch.cat([torch.tensor(p.obj_trans, device=dev).expand(PA, -1) for p in poses[1:]])
    xyz.append(torch.einsum('bij,bj->bi', qmat(orot), loc_x) + otr)
    rot.append(torch.nn.functional.normalize(qmul(orot, loc_r)))
    for m, p in zip(models[1:], poses[1:]):
        sca.append(torch.exp(m.scaling)); opa.append(torch.sigmoid(m.opacity))
        base = torch.tensor(idft_weights(p.fourier_time, FD), device=dev)
        fea.append(torch.cat([torch.sum(m.features_dc * base[..., None], 1, keepdim=True), m.features_rest], 1))
    return torch.cat(xyz), torch.cat(sca), torch.cat(rot), torch.cat(opa), torch.cat(fea)


def torch_normals(x, s, r, campos):
    """GaussianModel.get_normals (gaussian_model.py:256-269) on the composed tensors"""
    k = torch.argmin(s, dim=-1)
    n = qmat(r)[torch.arange(k.shape[0], device=dev), :, k]
    d = x - campos[None]
    d = d / d.norm(dim=1, keepdim=True)
    return torch.where(torch.sum(-d * n, dim=1, keepdim=True) >= 0, n, -n)


cams = [hz.trajectory_camera(f, device=dev) for f in range(args.calls + 2)]
rss = [GaussianRasterizationSettings(**hz.settings_kwargs(c, 1)) for c in cams]


def loss_of(c, d, al, f):
    return c.mean() + 0.1 * d.mean() + al.mean() + f.mean()


def train_torch(f, normals):
    x, s, r, o, sh = torch_compose(poses_at(f))
    feats = torch.cat(sems, 0)
    if normals:
        feats = torch.cat((torch_normals(x, s, r, rss[f].campos), feats), 1)
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    c, _, d, al, fp = GaussianRasterizer(rss[f])(means3D=x, means2D=m2d, opacities=o, shs=sh, scales=s, rotations=r,
                                                 semantics=feats)
    loss_of(c, d, al, fp).backward()


def train_fused(f, normals):
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    c, _, d, al, fp = ComposedRasterizer(rss[f]).forward_features(models, poses_at(f), sems, bool(normals), means2D=m2d)
    loss_of(c, d, al, fp).backward()


def zero_grads():
    for m in models:
        for t in m[:6]:
            t.grad = None
    for t in sems:
        t.grad = None


def one_rep(fn, normals):
    ts = []
    for k in range(args.calls + 2):
        zero_grads()
        ts.append(benchkit.once(fn, k, normals, events=False)["wall_us"] / 1e3)
    return median(ts[2:])     # two warm-up calls


result = {"what": "train step with feature planes, 1 M background + 10 actors x 10 k, 1920x1280, S = 15; per cell the "
                  "medians of %d repetitions of (median of %d synchronize-bracketed calls), ms" % (args.reps, args.calls),
          "cells": {}}
for normals in ((0, 1) if args.normals is None else (args.normals,)):
    cell = {}
    for name, fn in (("torch_composition_cat_classic_op", train_torch), ("forward_features", train_fused)):
        if args.only and (args.only == "fused") != (fn is train_fused):
            continue
        reps = [one_rep(fn, normals) for _ in range(args.reps)]
        cell[name] = {"median_ms": median(reps), "repetitions_ms": reps}
    if len(cell) == 2:
        cell["ratio"] = cell["torch_composition_cat_classic_op"]["median_ms"] / cell["forward_features"]["median_ms"]
    result["cells"]["F=%d (normals %s)" % (3 * normals + S, "on" if normals else "off")] = cell
benchkit.emit(result, args.out)
