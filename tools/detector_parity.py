"""Parity of the detector's network (gaussianrpg_amd/detector.py, csrc/detector.hip) on the GPU against the float64
truth of tests/detector_truth.py, next to the reference's own recorded distance (tests/golden/ref_detector.json):
per whole-network case and head the relative L2 distance, the worst element and the ratio to the reference's figure
(the tests' bar is 4); per convolution leaf case of tests/test_gpu_detector.py the worst error over the derived
per-element bound, for both tile shapes.  Prints one JSON line; --out FILE also writes it
(profiles/detector_parity.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import detector_truth as T
import test_gpu_detector as G
from gaussianrpg_amd import detector as D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    with open(os.path.join(T.GOLDEN, "ref_detector.json")) as f:
        golden = json.load(f)
    res = {"device": torch.cuda.get_device_name(0), "margin": G.MARGIN, "network": {}, "conv_leaf": {}}
    for case in T.CASES:
        spec, sd, x = T.case_inputs(case)
        heads64, _ = T.network64(spec, sd, x)
        heads = D.DetectorNet(spec, sd)(torch.from_numpy(x).to(dev))
        torch.cuda.synchronize()
        rows = []
        for l, (h, t) in enumerate(zip(heads, heads64)):
            ref = golden["cases"][case]["heads"][l]
            d = T.rel_l2(h.cpu(), t)
            rows.append({"rel_l2": d, "worst": T.worst(h.cpu(), t), "reference_rel_l2": ref[0], "reference_worst": ref[1],
                         "ratio": d / ref[0]})
        res["network"][case] = rows
    for name, (bs, c_in, c_out, k, s, hw, act, r_on, focus, up) in G.CONV_CASES.items():
        x, w, b, rs = G._case(sum(map(ord, name)), bs, c_in, c_out, k, hw, focus=focus)
        lh, lw = (hw[0] // 2, hw[1] // 2) if focus else hw
        r = rs.normal(0, 1, (bs, c_out, D.out_size(lh, k, s), D.out_size(lw, k, s))).astype(np.float32) if r_on else None
        want, bound = T.conv64(x, w, b, k, s, act, r, focus)
        row = {"K": c_in * k * k}
        for tile, tname in ((D.TILE_128, "tile128"), (D.TILE_64, "tile64")):
            out, _ = G.run_conv(dev, x, w, b, k, s, act, r, focus, up, tile)
            row[tname] = float(((out.double() - want).abs() / bound).max())
        res["conv_leaf"][name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
