"""Generate tests/golden/ref_nms.json + ref_nms.npz.  Needs a checkout of the reference (GaussianRPG); never run by a
test:

    python tests/golden/make_golden_nms.py <path to the reference>

Cuts ``non_max_suppression`` and ``xywh2xyxy`` out of the reference's utils/general.py and ``scale_coords`` and
``clip_coords`` out of its utils/torch_utils.py with ``ast`` (the modules themselves import torchvision, cv2 and
pandas, which are not installed here) and executes them on CPU torch.  Their namespace holds ``torch``, ``np``,
``time``, a ``LOGGER`` that records (the function warns when its wall-clock limit passes; the generator asserts that
no image was lost to it) and a stand-in for ``torchvision`` whose ``ops.nms`` is the greedy loop of torchvision's CPU
kernel in float32 torch operations -- THE ONE STEP NOT EXECUTED FROM THE REFERENCE.  Where torchvision imports, the
generator asserts that the stand-in equals ``torchvision.ops.nms`` on every case.

The files hold numbers only.  Inputs are not stored: a case names its builder in tests/nms_truth.py and the builder's
arguments (legacy numpy RandomState: stable), and records the sha256 of the input's bytes, the settings, and per image
what the reference returned: the [n, 6] rows of non_max_suppression and, where the case has a frame,
scale_coords(input_hw, det[:, :4], (H, W, 3)).round().
"""
import ast
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nms_truth as nt   # noqa: E402  (the input builders only)


# ---- the stand-in for torchvision.ops.nms ----

def _standin_nms(boxes, scores, iou_threshold):
    """torchvision/csrc/ops/cpu/nms_kernel.cpp, float32: stable descending order of the scores; area = (x2 - x1) *
    (y2 - y1); w = clamp(min(x2) - max(x1), 0), the same for h; box j is suppressed by a kept box i when
    inter / (area_i + area_j - inter) > thr.  The kernel makes that last comparison in double (a float IoU against
    the double threshold); so does this.  Returns the kept indices in descending score."""
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32
    n = boxes.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64)
    x1, y1, x2, y2 = boxes.unbind(1)
    areas = (x2 - x1) * (y2 - y1)
    order = scores.sort(stable=True, dim=0, descending=True)[1]
    suppressed = torch.zeros(n, dtype=torch.bool)
    keep = []
    for k in range(n):
        i = int(order[k])
        if suppressed[i]:
            continue
        keep.append(i)
        rest = order[k + 1:]
        w = torch.clamp(torch.minimum(x2[i], x2[rest]) - torch.maximum(x1[i], x1[rest]), min=0)
        h = torch.clamp(torch.minimum(y2[i], y2[rest]) - torch.maximum(y1[i], y1[rest]), min=0)
        inter = w * h
        ovr = inter / (areas[i] + areas[rest] - inter)
        assert ovr.dtype == torch.float32
        suppressed[rest[ovr.double() > float(iou_threshold)]] = True
    return torch.tensor(keep, dtype=torch.int64)


class _Ops:
    nms = staticmethod(_standin_nms)


class _Torchvision:
    ops = _Ops


class _Logger:
    def __init__(self):
        self.warnings = []

    def warning(self, msg):
        self.warnings.append(msg)


def _cut(path, names):
    with open(path) as f:
        tree = ast.parse(f.read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in fns) == sorted(names), (path, [n.name for n in fns])
    return compile(ast.Module(body=fns, type_ignores=[]), path, "exec")


def _reference(ref):
    logger = _Logger()
    ns = {"torch": torch, "np": np, "time": time, "torchvision": _Torchvision, "LOGGER": logger}
    exec(_cut(os.path.join(ref, "utils", "general.py"), ["non_max_suppression", "xywh2xyxy"]), ns)
    exec(_cut(os.path.join(ref, "utils", "torch_utils.py"), ["scale_coords", "clip_coords"]), ns)
    return ns, logger


# ---- the cases: name, builder, its arguments, settings, frame, note ----

def _cases():
    mp = "make_prediction"
    heavy = dict(N=1000, nc=4, n_cand=500, seed=9, clusters=12, jitter=10.0)
    out = [("defaults", mp, dict(N=1000, nc=3, n_cand=200, seed=31), {}, None, "")]
    for agnostic in (False, True):
        for classes in (None, [0, 2], [7]):
            out.append(("heavy_agnostic%d_classes%s" % (agnostic, "".join(map(str, classes or [])) or "None"), mp, heavy,
                        dict(agnostic=agnostic, classes=classes), None, "classes [7]: none of the head's"))
    out += [
        ("off_every_tile", mp, dict(N=2049, nc=65, n_cand=130, seed=2049), {}, None, ""),
        ("max_det_10", mp, dict(N=1000, nc=3, n_cand=400, seed=4), dict(max_det=10), None,
         "the reference truncates after NMS"),
        ("max_det_1", mp, dict(N=1000, nc=3, n_cand=400, seed=4), dict(max_det=1), None, ""),
        ("batch_3", mp, dict(N=333, nc=2, n_cand=[5, 100, 64], seed=8, bs=3), {}, None, ""),
        ("batch_2_one_empty", mp, dict(N=1000, nc=3, n_cand=[200, 0], seed=7, bs=2), {}, None,
         "the empty image is zeros((0, 6))"),
        ("max_nms_30000", "max_nms_case", dict(seed=21), {}, None,
         "the 200 isolated candidates with the lowest confidences are cut by the reference's max_nms = 30000"),
        ("frame_simulator", "frame_case", dict(h=nt.SIM[0], w=nt.SIM[1], seed=13), dict(max_det=1024), list(nt.SIM),
         "gain 1, pad (0, 11): mapped values land on halves"),
        ("frame_resizing", "frame_case", dict(h=nt.RESIZE[0], w=nt.RESIZE[1], seed=14), dict(max_det=1024),
         list(nt.RESIZE), ""),
    ]
    for t in (0.25, 0.3):
        for product in (False, True):
            out.append(("threshold_%s_%s" % (t, "product" if product else "objectness"), "threshold_case",
                        dict(t=t, product=product), dict(conf_thres=t), None,
                        "how CPU torch compares a float32 tensor with a Python threshold"))
    out.append(("nan_rows", "nan_case", {}, {}, None, "the NaN IoU is the stand-in's (depends on the stand-in)"))
    out.append(("nan_rows_mapped", "nan_case", {}, {}, list(nt.SIM), "depends on the stand-in for the NaN IoU"))
    return out


def _distinct_confidences(x, conf_thres):
    with np.errstate(all="ignore"):
        c = (x[:, 5:] * x[:, 4:5]).max(1)
        c = c[c >= np.float32(conf_thres)]
    return len(np.unique(c)) == len(c)


def _check_against_torchvision(p, kw):
    try:
        import torchvision
    except ImportError:
        return False
    for x in p:
        c = torch.from_numpy(x[x[:, 4] > kw.get("conf_thres", 0.25)].copy())
        if not len(c):
            continue
        boxes = torch.from_numpy(nt.xywh2xyxy(c[:, :4].numpy()))
        scores = c[:, 4].clone()
        thr = kw.get("iou_thres", 0.45)
        assert torch.equal(_standin_nms(boxes, scores, thr), torchvision.ops.nms(boxes, scores, thr))
    return True


def main(ref):
    arrays, rows, tv_checked = {}, [], False
    for name, builder, args, kw, frame, note in _cases():
        p = nt.build_input(builder, args)
        conf_thres = kw.get("conf_thres", 0.25)
        for x in p:
            assert _distinct_confidences(x, conf_thres), "%s: two candidates tie; the reference leaves ties open" % name
        ns, logger = _reference(ref)
        dets = ns["non_max_suppression"](torch.from_numpy(p.copy()), **kw)
        assert isinstance(dets, list) and len(dets) == p.shape[0]
        assert len(logger.warnings) == 0 or p.shape[0] == 1, "%s: the time limit cut the batch short" % name
        tv_checked = _check_against_torchvision(p, kw) or tv_checked
        counts = []
        for b, d in enumerate(dets):
            d = d.detach().clone()
            assert d.dtype == torch.float32 and d.ndim == 2 and d.shape[1] == 6
            arrays["%s/%d/det" % (name, b)] = d.numpy().copy()
            counts.append(int(d.shape[0]))
            if frame is not None:
                h, w, H, W = frame
                m = ns["scale_coords"]((h, w), d[:, :4].clone(), (H, W, 3)).round()
                arrays["%s/%d/mapped" % (name, b)] = m.numpy().copy()
        rows.append(dict(name=name, builder=builder, args=args, settings=kw, frame=frame, note=note, counts=counts,
                         depends_on_standin_nan=name.startswith("nan_rows"),
                         sha256=hashlib.sha256(p.tobytes()).hexdigest(), shape=list(p.shape)))
        print("%-36s %s -> %s" % (name, list(p.shape), counts))

        # what each case is there to show, asserted on the reference's own output
        if name == "max_nms_30000":
            x = p[0]
            assert int((x[:, 4] > np.float32(0.25)).sum()) == 30200
            got = arrays[name + "/0/det"]
            assert len(got) < 300 and not (got[:, 1] >= nt.MAX_NMS_ISOLATED_Y - 20).any(), "isolated boxes in the output"
            cand = np.nonzero(x[:, 4] > np.float32(0.25))[0]
            order = cand[np.argsort(-x[cand, 4], kind="stable")]
            boxes = torch.from_numpy(nt.xywh2xyxy(x[order, :4]))
            uncut = _standin_nms(boxes, torch.from_numpy(x[order, 4].copy()), 0.45)[:300]
            n_iso = int((x[order[uncut.numpy()], 1] >= nt.MAX_NMS_ISOLATED_Y).sum())
            assert n_iso > 0, "without the cut the isolated boxes must be kept"
            print("    without the max_nms cut: %d kept, %d of them isolated" % (len(uncut), n_iso))
        if frame is not None and not name.startswith("nan"):
            h, w, H, W = frame
            d, m = arrays[name + "/0/det"], arrays[name + "/0/mapped"]
            gain, px, py = nt.frame_map(h, w, H, W)
            raw = (d[:, :4].astype(np.float64) - [px, py, px, py]) / gain
            assert (raw[:, [0, 2]] < 0).any() and (raw[:, [0, 2]] > W).any(), "x clamps do not bind"
            assert (raw[:, [1, 3]] < 0).any() and (raw[:, [1, 3]] > H).any(), "y clamps do not bind"
            assert m.min() == 0 and m[:, [0, 2]].max() == W and m[:, [1, 3]].max() == H
            if gain == 1.0:
                inside = (raw > 0) & (raw < [W, H, W, H])
                assert (np.abs(raw - np.floor(raw) - 0.5)[inside] == 0).any(), "no mapped value lands on a half"

    source = ("utils/general.py (non_max_suppression, xywh2xyxy) and utils/torch_utils.py (scale_coords, clip_coords) "
              "of the reference, cut with ast and executed on CPU torch %s; torchvision.ops.nms is a stand-in (greedy "
              "loop of torchvision's CPU kernel in float32 torch operations), the one step not executed from the "
              "reference; stand-in compared with torchvision.ops.nms: %s" % (
                  torch.__version__.split("+")[0], "yes, equal on every case" if tv_checked else
                  "no (torchvision not installed where this was generated)"))
    with open(os.path.join(HERE, "ref_nms.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_nms.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
