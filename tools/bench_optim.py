"""The tail of the reference's training iteration, PyTorch against the fused HIP path (gaussianrpg_amd.optim):

* optimizer.step(): one torch.optim.Adam per model (7 parameter groups each, lr = 0, eps = 1e-15 at optimizer level,
  torch's default device path) against fused_adam_step over FusedAdam instances of the same tensors;
* set_max_radii2D + add_densification_stats (street_gaussian_model.py:555-578) model by model in PyTorch against
  densification_stats_update;

at (a) config 5: one model, P = 1 M, SH degree 1 (23 floats per Gaussian) and (b) the composition bench's scene:
1.9 M background + 10 actors x 10 k, 11 optimizers.  Every timed call sits between two device synchronisations
(CUDA events); a figure is the median of --steps calls after --warmup, taken --reps times: the JSON holds the median
of those medians and their spread (min, max).  --only fused runs nothing but the fused calls (for a kernel trace).
Prints one JSON line."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from gaussianrpg_amd.optim import FusedAdam, densification_stats_update, fused_adam_step

TAILS = ((3,), (1, 3), (3, 3), (1,), (3,), (4,), (0,))          # xyz f_dc f_rest opacity scaling rotation semantic
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")
LRS = (1.6e-4, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001, 0.0)
FLOATS_PER_GAUSSIAN = 23


def make_models(sizes, cls, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    models = []
    for P in sizes:
        params = [torch.nn.Parameter(torch.randn((P,) + t, generator=g).to(dev)) for t in TAILS]
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)
        opt = cls([{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(params, LRS, NAMES)], lr=0.0, eps=1e-15)
        models.append((params, opt))
    return models


def repeated(fn, steps, warmup, reps):
    meds = benchkit.windows({"fn": fn}, reps, steps, warmup, again=2, wall=False)["fn"]["device_us"]
    return benchkit.spread([us / 1e3 for us in meds], unit="ms")


def torch_densify(viewspace_grad, radii, ranges, models):
    """The reference's two methods, model by model (inclusive ranges there, half-open here)."""
    visibility_filter = radii > 0
    radii_f = radii.float()
    for (start, end), m in zip(ranges, models):
        vis = visibility_filter[start:end]
        r = radii_f[start:end]
        m["max_radii2D"][vis] = torch.max(m["max_radii2D"][vis], r[vis])
    for (start, end), m in zip(ranges, models):
        vis = visibility_filter[start:end]
        g = viewspace_grad[start:end]
        m["accum"][vis, 0:1] += torch.norm(g[vis, :2], dim=-1, keepdim=True)
        m["accum"][vis, 1:2] += torch.norm(g[vis, 2:], dim=-1, keepdim=True)
        m["denom"][vis] += 1


def bench_size(tag, sizes, args, dev, out):
    elements = FLOATS_PER_GAUSSIAN * sum(sizes)
    out[tag + "_models"] = len(sizes)
    out[tag + "_gaussians"] = sum(sizes)
    out[tag + "_adam_elements"] = elements
    out[tag + "_adam_hbm_floor_us_at_8TBs"] = 28.0 * elements / 8e12 * 1e6
    fused = make_models(sizes, FusedAdam, dev)
    fused_opts = [o for _, o in fused]
    out[tag + "_adam_fused"] = repeated(lambda: fused_adam_step(fused_opts), args.steps, args.warmup, args.reps)
    if args.only != "fused":
        ref = make_models(sizes, torch.optim.Adam, dev)

        def torch_step():
            for _, o in ref:
                o.step()
        out[tag + "_adam_torch"] = repeated(torch_step, args.steps, args.warmup, args.reps)
        del ref
    # densification statistics over the composed frame
    P = sum(sizes)
    g = torch.Generator().manual_seed(1)
    grad = torch.randn(P, 3, generator=g).to(dev)
    radii = torch.randint(1, 100, (P,), generator=g, dtype=torch.int32)
    radii[torch.rand(P, generator=g) < 0.4] = 0
    radii = radii.to(dev)
    ranges, s = [], 0
    for n in sizes:
        ranges.append((s, s + n))
        s += n
    stats = [{"accum": torch.zeros(n, 2, device=dev), "denom": torch.zeros(n, 1, device=dev),
              "max_radii2D": torch.zeros(n, device=dev)} for n in sizes]
    lists = [[m[k] for m in stats] for k in ("accum", "denom", "max_radii2D")]
    out[tag + "_densify_fused"] = repeated(lambda: densification_stats_update(grad, radii, ranges, *lists),
                                           args.steps, args.warmup, args.reps)
    if args.only != "fused":
        out[tag + "_densify_torch"] = repeated(lambda: torch_densify(grad, radii, ranges, stats),
                                               args.steps, args.warmup, args.reps)
    del fused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "fused"), default="all")
    args = ap.parse_args()
    benchkit.require_gpu("bench_optim")
    dev = torch.device("cuda:0")
    out = {"bench": "tools/bench_optim.py: optimizer.step() and densification statistics, PyTorch against fused HIP",
           "steps": args.steps, "reps": args.reps}
    bench_size("config5_P1M", [1_000_000], args, dev, out)
    bench_size("street_1p9M_10x10k", [1_900_000] + [10_000] * 10, args, dev, out)
    benchkit.emit(out)


if __name__ == "__main__":
    main()
