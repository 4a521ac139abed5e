"""Parity of the LPIPS backward (gaussianrpg_amd/lpips.py ``LPIPS.loss``, csrc/lpips_bwd.hip) on the GPU against the
conditional float64 truth of tests/lpips_bwd_truth.py at the HIP forward's own decisions, next to the reference's own
recorded distance (tests/golden/ref_lpips_bwd.json): per case the gradient's relative L2 distance and worst element
and their ratios to the reference's figures (the tests' bar for both is 4), and how many ReLU decisions of the HIP
forward differ from float64's own; per leaf case of tests/test_gpu_lpips_bwd.py the worst error over the derived bound.
Prints one JSON line; --out FILE also writes it (profiles/lpips_bwd_parity.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import benchkit
import lpips_bwd_truth as B
import lpips_truth as T
import test_gpu_lpips_bwd as G
from gaussianrpg_amd import lpips as LP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    benchkit.require_gpu("lpips_bwd_parity")
    dev = torch.device("cuda:0")
    with open(os.path.join(T.GOLDEN, "ref_lpips_bwd.json")) as f:
        golden = json.load(f)
    res = {"device": torch.cuda.get_device_name(0), "margin": B.MARGIN, "cases": {}, "conv_leaf": {}, "pool_leaf": {},
           "distance_leaf": {}}
    for case in T.CASES:
        net, features, lin, x, y = T.case_inputs(case)
        val, g, truth, xd, yd = G.run_case(dev, case)
        rel, worst = B.figures(g, truth)
        acc = B.acceptance(golden["cases"][case], g, truth)
        masks, _ = B.decisions_of(net, [a.cpu() for a in G.crit_of(net).train_activations(xd, yd)])
        own = B.forward64(net, features, x)["masks"]
        res["cases"][case] = {"rel_l2": rel, "worst": worst, "reference_rel_l2": golden["cases"][case]["rel_l2"],
                              "reference_worst": golden["cases"][case]["worst"], "rel_l2_ratio": acc["rel_l2"],
                              "worst_ratio": acc["worst"], "truth_max": float(truth.abs().max()),
                              "relu_decisions_unlike_float64": sum(int((a != b).sum()) for a, b in zip(masks, own)),
                              "loss_equals_distances": bool(torch.equal(val, G.crit_of(net).distances(xd, yd).cpu()))}
    for name, (bs, c_out, c_in, k, s, p, hw, epi) in G.CONV_CASES.items():
        g, w, act, tap = G.conv_inputs(name)
        want, bound = B.conv_bwd(g, w, k, s, p, hw, mask=act > 0 if epi.startswith("relu") else None,
                                 tap=tap if epi == "relu_tap" else None, std=epi == "std")
        res["conv_leaf"][name] = {"K": c_out * (-(-k // s)) ** 2,
                                  "tile128": G.worst_ratio(G.run_conv_bwd(dev, name, LP.TILE_128, g, w, act, tap), want, bound),
                                  "tile64": G.worst_ratio(G.run_conv_bwd(dev, name, LP.TILE_64, g, w, act, tap), want, bound)}
    for k, hw in ((3, (7, 7)), (3, (8, 11)), (3, (16, 22)), (2, (3, 5)), (2, (24, 40))):
        act, g, tap = G.pool_inputs(k, hw, 50 + hw[0] + hw[1] + k)
        want, bound = B.pool_bwd(act, g, k, tap=tap)
        got = LP.max_pool_backward(torch.from_numpy(act).to(dev), torch.from_numpy(g).to(dev), k, tap=torch.from_numpy(tap).to(dev))
        res["pool_leaf"]["k%d_%dx%d" % (k, hw[0], hw[1])] = G.worst_ratio(got.cpu(), want, bound)
    for c in (64, 192, 384, 256, 512):
        for hw in ((1, 1), (7, 7), (16, 22)):
            f, w, gp = G.distance_inputs(c, hw, c + hw[0])
            want, bound = B.distance_bwd(f[:2], f[2:], w, gp)
            res["distance_leaf"]["c%d_%dx%d" % (c, hw[0], hw[1])] = G.worst_ratio(G.run_distance_bwd(dev, f, w, gp), want, bound)
    benchkit.emit(res, args.out)


if __name__ == "__main__":
    main()
