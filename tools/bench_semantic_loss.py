"""The reference's semantic training term (train.py:129-143: the host-synchronising torch.all(gt == -1) guard, then
F.cross_entropy(..., ignore_index=-1); with semantic_mode 'probabilities' the normalise + log of
street_gaussian_renderer.py:248-256 in front) as PyTorch code against the fused HIP path
(gaussianrpg_amd.loss.semantic_loss), forward + backward, at 1920x1280 with S in {3, 15, 19, 32}, both modes,
20 % of the labels ignored.  Each entry holds forward ms, backward ms and ms for both: the median of --steps timed
iterations (device events, after --warmup).  For the fused path also the bytes the algorithm needs per call,
(4 S + sizeof(target) + 4) n forward and (8 S + sizeof(target) + 4) n backward, the achieved
GB/s over the event time and its share of the 8 TB/s floor; "backward_bytes_moved" and "backward_moved_gbs" count
what the backward really moves: it reads sem and the logsumexp only at valid pixels.  The event times include
the launches and, forward, the tiny reduce kernel, so the kernel-only share is a little higher.  Prints one JSON line."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import benchkit
from benchkit import median
from gaussianrpg_amd import loss as fused_loss

HBM_PEAK_GBS = 8000.0
IGNORED = 0.2


def torch_semantic(semantic, gt, mode):
    """train.py:129-143 behind street_gaussian_renderer.py:248-256."""
    if mode == "probabilities":
        semantic = semantic / (torch.sum(semantic, dim=0, keepdim=True) + 1e-8)
        semantic = torch.log(semantic + 1e-8)
    if torch.all(gt == -1):
        return torch.zeros((), device=semantic.device)
    return torch.nn.functional.cross_entropy(input=semantic.unsqueeze(0), target=gt, ignore_index=-1, reduction="mean")


def fused_semantic(semantic, gt, mode):
    return fused_loss.semantic_loss(semantic, gt, mode=mode)


def _inputs(S, H, W, mode, dev):
    g = torch.Generator().manual_seed(S + H)
    sem = torch.randn(S, H, W, generator=g) if mode == "logits" else torch.rand(S, H, W, generator=g) * 0.98 + 0.01
    gt = torch.randint(0, S, (1, H, W), generator=g)
    gt[torch.rand(1, H, W, generator=g) < IGNORED] = -1
    return sem.to(dev), gt.to(dev)


def time_loss(fn, sem, gt, mode, steps, warmup):
    fw, bw, both = [], [], []
    x = sem.clone().requires_grad_(True)
    for it in range(warmup + steps):
        x.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        l = fn(x, gt, mode)
        e[1].record()
        l.backward()
        e[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            both.append(e[0].elapsed_time(e[2]))
    return {"forward_ms": median(fw), "backward_ms": median(bw), "fwd_bwd_ms": median(both)}


def fused_bytes(S, n, n_valid, target_bytes=8):
    """(forward, backward, backward as moved) bytes: every plane once, the label, the logsumexp plane; the
    backward writes every gradient element and reads sem and the logsumexp only at valid pixels."""
    fwd = (4 * S + target_bytes + 4) * n
    bwd = (8 * S + target_bytes + 4) * n
    moved = (4 * S + target_bytes) * n + (4 * S + 4) * n_valid
    return fwd, bwd, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 15, 19, 32])
    args = ap.parse_args()
    benchkit.require_gpu("bench_semantic_loss")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    out = {"bench": "tools/bench_semantic_loss.py: train.py semantic cross-entropy, fwd + bwd, %dx%d, %d %% ignored"
                    % (W, H, round(100 * IGNORED)), "steps": args.steps}
    for S in args.channels:
        for mode in ("logits", "probabilities"):
            sem, gt = _inputs(S, H, W, mode, dev)
            n_valid = int((gt >= 0).sum())
            for name, fn in (("torch", torch_semantic), ("fused", fused_semantic)):
                r = time_loss(fn, sem, gt, mode, args.steps, args.warmup)
                if name == "fused":
                    fb, bb, bm = fused_bytes(S, H * W, n_valid)
                    r["forward_bytes"], r["backward_bytes"], r["backward_bytes_moved"] = fb, bb, bm
                    r["backward_moved_gbs"] = bm / r["backward_ms"] * 1e-6
                    r["forward_gbs"] = fb / r["forward_ms"] * 1e-6
                    r["backward_gbs"] = bb / r["backward_ms"] * 1e-6
                    r["forward_share_of_8tbs"] = r["forward_gbs"] / HBM_PEAK_GBS
                    r["backward_share_of_8tbs"] = r["backward_gbs"] / HBM_PEAK_GBS
                out["S%d_%s_%s" % (S, mode, name)] = r
            t, f = out["S%d_%s_torch" % (S, mode)], out["S%d_%s_fused" % (S, mode)]
            out["S%d_%s_speedup" % (S, mode)] = t["fwd_bwd_ms"] / f["fwd_bwd_ms"]
    benchkit.emit(out)


if __name__ == "__main__":
    main()
