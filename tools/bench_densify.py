"""densify_and_prune of all models: the reference's PyTorch sequence (gaussianrpg_amd.harness.
densify_and_prune_reference, model by model, without its torch.cuda.empty_cache()) against the fused HIP call
(gaussianrpg_amd.optim.densify_and_prune), on the same tensors, the same noise and the reference's default thresholds
(config.py:57-67), at (a) one model, P = 1 M and (b) 1.9 M background + 10 actors x 10 k, SH degree 1 (23 floats per
Gaussian, parameter + two moments = 276 B).  The statistics are drawn so that a few per cent of the rows clone, split
and are pruned.

The two sides alternate in one process: per repetition --steps timed calls of each side, every call between two device
synchronisations (CUDA events), on optimizers rebuilt, outside the timed span, over the same input tensors (a call
replaces its optimizer's parameters; the inputs are not modified).  A figure is the median of the repetitions' medians with its spread.
Host synchronisations are counted with torch's sync debug mode in one extra call per side; the fused call's own wait
(the plan's, inside the library, invisible to torch) is added by hand.  Kernel times come from a run of their own under
rocprofv3 --kernel-trace --stats with --only fused.  Prints one JSON line."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from benchkit import count_syncs
from gaussianrpg_amd import harness as hz
from gaussianrpg_amd.optim import DensifyModel, DensifyRule, FusedAdam, densify_and_prune

TAILS = ((3,), (1, 3), (3, 3), (1,), (3,), (4,), (0,))          # xyz f_dc f_rest opacity scaling rotation semantic
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic")
FLOATS_PER_GAUSSIAN = 23
BYTES_PER_ROW = 3 * 4 * FLOATS_PER_GAUSSIAN                      # parameter, exp_avg, exp_avg_sq


def make_inputs(P, k, dev, seed):
    """Model k's tensors on the device: ~3 % of the rows clone, ~1 % split, ~4 % are transparent, ~1 % big."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)          # noqa: E731
    t = {n: torch.randn((P,) + tail, generator=g, device=dev) for n, tail in zip(NAMES, TAILS)}
    extent = 20.0 if k == 0 else 4.0                                  # dense threshold 0.01 extent, big 0.1 extent
    lo, hi = math.log(0.002 * extent), math.log(0.02 * extent)
    base = torch.exp(lo + (hi - lo) * rnd(P, 1))
    base = torch.where(rnd(P, 1) < 0.01, torch.full_like(base, 0.15 * extent), base)
    t["scaling"] = torch.log(base * (0.5 + 0.5 * rnd(P, 3)))
    t["opacity"] = torch.where(rnd(P, 1) < 0.04, torch.full((P, 1), -7.0, device=dev), 4.0 * rnd(P, 1) - 1.0)
    t["xyz"] = (2.0 * rnd(P, 3) - 1.0) * (3.0 * extent if k == 0 else 0.3 * extent)
    denom = torch.randint(1, 20, (P, 1), generator=g, device=dev).float()
    grads = 0.0002 * torch.exp(torch.randn(P, 2, generator=g, device=dev) - 1.7)      # P(g >= 0.0002) ~ 4.5 %
    moments = {n: (torch.randn_like(t[n]), torch.rand_like(t[n])) for n in NAMES}
    if k == 0:
        rule = DensifyRule.background(0.0002, 0.005, True, scene_radius=extent, sphere_center=(0.0, 0.0, 0.0),
                                      sphere_radius=extent)
    else:
        rule = DensifyRule.actor(0.0002, 0.005, True, extent=extent, box_min=(-0.6 * extent,) * 3,
                                 box_max=(0.6 * extent,) * 3)
    return {"tensors": t, "moments": moments, "accum": grads * denom, "denom": denom, "rule": rule,
            "split_noise": torch.randn(P, 2, 3, generator=g, device=dev),
            "box_noise": torch.randn(P, 4, 2, 3, generator=g, device=dev) if k else None}


def fused_models(inputs):
    models = []
    for m in inputs:
        groups = [{"params": [torch.nn.Parameter(m["tensors"][n])], "lr": 1e-3, "name": n} for n in NAMES]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15)
        for grp in opt.param_groups:
            ea, es = m["moments"][grp["name"]]
            opt.state[grp["params"][0]] = {"step": torch.tensor(100.0), "exp_avg": ea, "exp_avg_sq": es}
        models.append(DensifyModel(opt, m["accum"], m["denom"], m["rule"], m["split_noise"], m["box_noise"]))
    return models


def run_fused(inputs):
    return densify_and_prune(fused_models(inputs))


def run_reference(inputs):
    return [hz.densify_and_prune_reference(m["tensors"], m["moments"], m["accum"], m["denom"], m["rule"],
                                           m["split_noise"], m["box_noise"]) for m in inputs]


def timed(fn, prepare, steps, warmup):
    """Median ms over `steps` calls of fn(prepare()); prepare() (the optimizers of one call) is not timed."""
    return benchkit.medians(benchkit.timed(fn, steps, warmup, prepare=prepare, wall=False))["device_us"] / 1e3


def bench_size(tag, sizes, args, dev, out):
    inputs = [make_inputs(P, k, dev, 10 + k) for k, P in enumerate(sizes)]
    res = run_fused(inputs)
    torch.cuda.synchronize()
    rows_in, rows_out = sum(sizes), sum(r.src_index.numel() for r in res)
    scal = {k: sum(r.scalars[k] for r in res) for k in res[0].scalars}
    out[tag] = o = {"models": len(sizes), "rows_in": rows_in, "rows_out": rows_out, "scalars": scal}
    if args.only != "fused":
        ref = run_reference(inputs)
        same = all(torch.equal(a["src_index"], b.src_index) for a, b in zip(ref, res))
        o["same_rows_as_reference_sequence"] = bool(same)
        o["max_abs_diff_vs_reference_sequence"] = max(
            float((a["tensors"][n] - b.params[n].detach()).abs().max()) if b.params[n].numel() else 0.0
            for a, b in zip(ref, res) for n in NAMES)
        del ref
    del res
    # bytes the apply pass must move: every source row read once, every output row written once (parameter and two
    # moments, DESIGN.md section 13's 23 floats), the class byte, src_index and the three fresh statistics
    o["apply_bytes"] = BYTES_PER_ROW * (rows_in + rows_out) + rows_in + 20 * rows_out
    o["apply_floor_us_at_8TBs"] = o["apply_bytes"] / 8e12 * 1e6
    o["apply_floor_us_at_6p3TBs"] = o["apply_bytes"] / 6.3e12 * 1e6
    fused, refs = [], []
    for r in range(args.reps):
        fused.append(timed(densify_and_prune, lambda: fused_models(inputs), args.steps, args.warmup if r == 0 else 1))
        if args.only != "fused":
            refs.append(timed(run_reference, lambda: inputs, args.steps, args.warmup if r == 0 else 1))
    o["fused"] = benchkit.spread(fused, unit="ms")
    o["fused"]["host_syncs"] = count_syncs(lambda: run_fused(inputs)) + 1        # + the plan's own stream wait
    if args.only != "fused":
        o["reference_sequence"] = benchkit.spread(refs, unit="ms")
        o["reference_sequence"]["host_syncs"] = count_syncs(lambda: run_reference(inputs))
        o["speedup"] = o["reference_sequence"]["ms"] / o["fused"]["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "fused"), default="all")
    ap.add_argument("--sizes", choices=("all", "a", "b"), default="all")
    args = ap.parse_args()
    benchkit.require_gpu("bench_densify")
    dev = torch.device("cuda:0")
    out = {"bench": "tools/bench_densify.py: densify_and_prune, the reference's PyTorch sequence against fused HIP",
           "steps": args.steps, "reps": args.reps}
    if args.sizes in ("all", "a"):
        bench_size("config5_P1M", [1_000_000], args, dev, out)
    if args.sizes in ("all", "b"):
        bench_size("street_1p9M_10x10k", [1_900_000] + [10_000] * 10, args, dev, out)
    benchkit.emit(out)


if __name__ == "__main__":
    main()
