"""How far the device's object positions lie from the longdouble truth, next to the numpy float64 restatement's own
distance (tests/loop_truth.py, the cases of tests/test_gpu_ego_loop.py): per case and per group of cases the two maxima
and their ratio -- the figure tests/test_gpu_ego_loop.py::test_ranging_accuracy holds to 4.  Also the scenarios' logs
and camera rows: the number of elements that differ in any bit from the restatement (expected 0).  Prints one JSON
line; --out FILE also writes it (profiles/ego_loop_parity.json)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import benchkit
import loop_truth as lt
import test_gpu_ego_loop as tg
from gaussianrpg_amd import closed_loop as cl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    benchkit.require_gpu("ego_loop_parity")
    dev = torch.device("cuda:0")
    C = lt.Constants()
    ranging = cl.Ranging(C.K, C.extrinsics, C.cam_height, C.H, C.W, names=lt.NAMES)
    cases = tg.measure_ranging(dev, ranging, C)
    result = {"tool": "tools/ego_loop_parity.py", "device": torch.cuda.get_device_name(0),
              "what": "object positions: max |device - longdouble truth| and max |numpy float64 restatement - truth| in "
                      "metres, per case and per max_det group; bound: ratio <= 4",
              "cases": cases, "groups": {}, "scenarios": {}}
    for group in ("10", "64"):
        sel = [m for name, m in cases.items() if name.endswith("_" + group) and m["kept"]]
        e_dev, e_f64 = max(m["err_dev"] for m in sel), max(m["err_f64"] for m in sel)
        result["groups"]["max_det_" + group] = {"err_dev": e_dev, "err_f64": e_f64, "ratio": e_dev / e_f64,
                                                "positions": sum(m["kept"] for m in sel)}
    world = tg.World(dev)
    for name in lt.SCENARIOS:
        log, rows, ks, loop, want, poses, truth = tg.run_device(world, ranging, name, sky=True)
        result["scenarios"][name] = {"steps": len(log), "log_elements_differing": int((log.view(np.uint64) != want.view(np.uint64)).sum())}
    benchkit.emit(result, args.out)


if __name__ == "__main__":
    main()
