"""Generate tests/golden/ref_detect.json + ref_detect.npz.  Needs a checkout of the reference (GaussianRPG); never run
by a test:

    python tests/golden/make_golden_detect.py <path to the reference>

Cuts class ``Detect`` out of the reference's models/yolo.py with ``ast`` (the module itself imports the whole model
zoo; the class needs only ``torch`` and ``torch.nn``), builds it with the case's anchors, replaces its 1x1 convs by
identities, and runs it in ``eval()`` on CPU torch on the case's heads: what comes back is the inference branch of
``Detect.forward`` itself.  Its prediction then goes through the reference's ``non_max_suppression`` as
make_golden_nms.py cuts it out (the same stand-in for torchvision.ops.nms, the one step not executed from the
reference).

The files hold numbers only.  Inputs are not stored: a case names its builder in tests/detect_truth.py and the
builder's arguments (legacy numpy RandomState: stable) and records the sha256 of the input's bytes.  Per case: the
reference's own distance from the float64 truth of detect_truth.decode per column group (relative L2, worst element);
its prediction where that keeps the fixture small (PRED_LIMIT bytes); for the planted cases its detections per
image and their distance from the truth's detections.  The planted cases keep every decision DECISION_MARGIN from
its threshold on the float64 truth: asserted here, and again by tests/test_detect_host.py.
"""
import ast
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import detect_truth as dt          # noqa: E402
from make_golden_nms import _reference   # noqa: E402

PRED_LIMIT = 128 * 1024
PLANTED = [(80, (64, 96), 2, 6), (3, (96, 160), 1, 16), (1, (64, 96), 1, 6), (80, (160, 256), 1, 40)]


def _detect_class(ref):
    path = os.path.join(ref, "models", "yolo.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Detect"]
    assert len(cls) == 1
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), ns)
    return ns["Detect"]


def reference_pred(Detect, heads, geom):
    anchors = [[float(v) for v in geom.anchor_grid[l].reshape(-1)] for l in range(geom.nl)]
    m = Detect(nc=geom.nc, anchors=anchors, ch=())
    m.m = torch.nn.ModuleList(torch.nn.Identity() for _ in range(geom.nl))
    m.stride = torch.tensor([float(s) for s in geom.stride])
    m.eval()
    assert m.na == geom.na and m.nl == geom.nl and m.inplace
    assert np.array_equal(m.anchor_grid.numpy().reshape(geom.nl, geom.na, 2), geom.anchor_grid)
    with torch.no_grad():
        pred, _ = m([torch.from_numpy(h.copy()) for h in heads])
    assert pred.dtype == torch.float32
    return pred.numpy().copy()


def _cases():
    out = [("dense_64x96_bs2_nc80", "dense_heads", dict(nc=80, hw=[64, 96], bs=2, seed=1)),
           ("dense_96x160_nc3", "dense_heads", dict(nc=3, hw=[96, 160], bs=1, seed=2)),
           ("dense_5x7_one_level_na1_nc1", "dense_heads", dict(nc=1, hw=[40, 56], bs=1, seed=3, strides=[8], na=1)),
           ("dense_nl4_nc65", "dense_heads", dict(nc=65, hw=[128, 192], bs=1, seed=4, strides=[8, 16, 32, 64])),
           ("dense_160x256_nc80", "dense_heads", dict(nc=80, hw=[160, 256], bs=1, seed=5))]
    for nc, hw, bs, clusters in PLANTED:
        seed = dt.first_good_seed(nc, hw, bs, clusters)
        out.append(("planted_%dx%d_bs%d_nc%d" % (hw[0], hw[1], bs, nc), "planted",
                    dict(nc=nc, hw=list(hw), bs=bs, clusters=clusters, seed=seed)))
    return out


def main(ref):
    Detect = _detect_class(ref)
    arrays, rows = {}, []
    for name, builder, args in _cases():
        heads, geom = dt.build_input(builder, args)
        truth = dt.decode(heads, geom)
        pred = reference_pred(Detect, heads, geom)
        assert pred.shape == truth.shape
        figures = {g: list(dt.errors(pred[..., s], truth[..., s])) for g, s in dt.GROUPS.items()}
        row = dict(name=name, builder=builder, args=args, shape=list(pred.shape), figures=figures,
                   sha256=hashlib.sha256(dt.input_bytes(heads, geom)).hexdigest(), pred_stored=pred.nbytes <= PRED_LIMIT)
        if row["pred_stored"]:
            arrays[name + "/pred"] = pred
        if builder == "planted":
            ok, worst, supp = dt.planted_ok(heads, geom)
            assert ok, (name, worst, supp)
            ns, logger = _reference(ref)
            dets = ns["non_max_suppression"](torch.from_numpy(pred.copy()))
            assert len(dets) == pred.shape[0] and not logger.warnings
            counts, det_figures = [], {"box": [0.0, 0.0], "conf": [0.0, 0.0]}
            got_all, want_all = [], []
            for b, d in enumerate(dets):
                d = d.numpy().copy()
                _, want, _ = dt.detections_image64(truth[b])
                assert d.shape == want.shape and np.array_equal(d[:, 5], want[:, 5]), name
                assert np.abs(d - want).max() < 1e-3, name          # the same rows in the same order
                arrays["%s/%d/det" % (name, b)] = d
                counts.append(int(d.shape[0]))
                got_all.append(d)
                want_all.append(want)
            got_all, want_all = np.concatenate(got_all), np.concatenate(want_all)
            det_figures = {"box": list(dt.errors(got_all[:, :4], want_all[:, :4])),
                           "conf": list(dt.errors(got_all[:, 4], want_all[:, 4]))}
            row.update(counts=counts, suppressed=supp, margins=worst, det_figures=det_figures)
        rows.append(row)
        print("%-32s %s stored=%s %s" % (name, list(pred.shape), row["pred_stored"], row.get("counts", "")))
        print("    " + "  ".join("%s %.2e/%.2e" % (g, *f) for g, f in figures.items()))
    source = ("class Detect of the reference's models/yolo.py, cut with ast, its convs replaced by identities, run in "
              "eval() on CPU torch %s; detections by the reference's non_max_suppression as tests/golden/"
              "make_golden_nms.py runs it (torchvision.ops.nms is its stand-in)" % torch.__version__.split("+")[0])
    with open(os.path.join(HERE, "ref_detect.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_detect.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
