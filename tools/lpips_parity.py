"""Parity of LPIPS (gaussianrpg_amd/lpips.py, csrc/lpips.hip) on the GPU against the float64 truth of
tests/lpips_truth.py, next to the reference's own recorded distance (tests/golden/ref_lpips.json): per net and tap the
relative L2 distance of the per-pixel maps pooled over the net's cases and its ratio to the reference's figure, per case
and pair the value's error over the reference's summed mean absolute map error (the tests' bar for both is 4); per
convolution and distance leaf case of tests/test_gpu_lpips.py the worst error over the derived bound.  Prints one JSON
line; --out FILE also writes it (profiles/lpips_parity.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import benchkit
import lpips_truth as T
import test_gpu_lpips as G
from gaussianrpg_amd import lpips as LP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    benchkit.require_gpu("lpips_parity")
    dev = torch.device("cuda:0")
    with open(os.path.join(T.GOLDEN, "ref_lpips.json")) as f:
        golden = json.load(f)
    res = {"device": torch.cuda.get_device_name(0), "margin": T.MARGIN, "nets": {}, "cases": {}, "conv_leaf": {},
           "distance_leaf": {}}
    for net in ("alex", "vgg"):
        results = {}
        for case, row in T.CASES.items():
            if row[0] == net:
                maps, values, _, truth, _, _ = G.run_case(dev, case)
                results[case] = (maps, values, truth)
        acc = T.acceptance(net, golden, results)
        ref = golden["nets"][net]
        res["nets"][net] = {"map_rel_l2": [r * g for r, g in zip(acc["map_ratio"], ref["map_rel_l2"])],
                            "reference_map_rel_l2": ref["map_rel_l2"], "map_ratio": acc["map_ratio"],
                            "reference_summed_mean_abs": sum(ref["map_mean_abs"])}
        for case, ratios in acc["value_ratio"].items():
            res["cases"][case] = {"values": results[case][1].tolist(), "truth_values": results[case][2]["values"].tolist(),
                                  "reference_total": golden["cases"][case]["reference"], "value_ratio": ratios}
    for name, (bs, c_in, c_out, k, s, p, hw, z) in G.CONV_CASES.items():
        x, w, b = G.conv_inputs(name)
        want, bound = T.conv_relu64(x, w, b, k, s, p, z)
        row = {"K": c_in * k * k}
        for tile, tname in ((LP.TILE_128, "tile128"), (LP.TILE_64, "tile64")):
            row[tname] = float(((G.run_conv(dev, name, tile).double() - want).abs() / bound).max())
        res["conv_leaf"][name] = row
    for c in (64, 192, 384, 256, 512):
        for hw in ((1, 1), (7, 7), (16, 22)):
            f, w = G.distance_inputs(c, hw, c + hw[0])
            s64, m64, e_s, e_m = T.distance64(f[:2], f[2:], w)
            mean, smap = LP.tap_distance(torch.from_numpy(f).to(dev), torch.from_numpy(w).to(dev))
            res["distance_leaf"]["c%d_%dx%d" % (c, hw[0], hw[1])] = {
                "map": float(((smap.cpu().double() - s64).abs() / e_s).max()),
                "mean": float(((mean.cpu().double() - m64).abs() / e_m).max())}
    benchkit.emit(res, args.out)


if __name__ == "__main__":
    main()
