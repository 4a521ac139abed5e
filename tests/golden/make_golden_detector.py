"""Generate tests/golden/ref_detector.json + ref_detector.npz.  Needs a checkout of the reference (GaussianRPG); never
run by a test:

    python tests/golden/make_golden_detector.py <path to the reference>

The reference's model zoo imports cv2, pandas and requests at module level, so the modules cannot be imported.  This
script cuts ``autopad``, ``Conv``, ``Bottleneck``, ``C3``, ``SPP``, ``Focus``, ``Concat`` (models/common.py),
``Detect`` and ``parse_model`` (models/yolo.py), ``make_divisible`` (utils/general.py) and ``fuse_conv_and_bn``
(utils/torch_utils.py) out of the reference with ``ast`` -- as make_golden_detect.py does for ``Detect`` -- and runs
them on CPU torch: ``parse_model`` builds the network from the yaml, the seeded weights of tests/detector_truth.py
are loaded with ``load_state_dict(strict=True)`` (which pins every key name and shape), every ``Conv`` is fused the way
``Model.fuse`` does, and the layers are walked the way ``Model.forward_once`` does (``m.f``, the save list) with
``Detect`` in training mode, so that it returns its conv outputs: the heads.

The files hold numbers and names only.  Inputs are not stored: a case names its builder arguments in
tests/detector_truth.py and records the sha256 of the input's and the weights' bytes.  Per whole-network case: the
state dict's keys and shapes (unfused and fused), the reference's float32 heads, and the reference's own distance from
the float64 truth (detector_truth.network64) per head and per layer, relative L2 and worst element.  Per leaf case: the
output of the reference's own module (Conv with the weights set, Focus, SPP's pools).
"""
import ast
import json
import logging
import os
import sys
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detector_truth as T          # noqa: E402

WANTED = {"models/common.py": ("autopad", "Conv", "Bottleneck", "C3", "SPP", "Focus", "Concat"),
          "models/yolo.py": ("Detect", "parse_model"),
          "utils/general.py": ("make_divisible",),
          "utils/torch_utils.py": ("fuse_conv_and_bn",)}
ABSENT = ("GhostConv", "GhostBottleneck", "DWConv", "MixConv2d", "CrossConv", "BottleneckCSP", "C3TR", "Contract", "Expand")


def reference_namespace(ref):
    import math
    ns = {"torch": torch, "nn": nn, "math": math, "logger": logging.getLogger("golden"), "deepcopy": deepcopy}
    for name in ABSENT:                       # parse_model names them in a list; none is in the yaml
        ns[name] = type(name, (), {})
    for rel, names in WANTED.items():
        path = os.path.join(ref, rel)
        with open(path) as f:
            tree = ast.parse(f.read())
        body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
        assert sorted(n.name for n in body) == sorted(names), (rel, [n.name for n in body])
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def build_reference(ns, cfg, spec, state_dict):
    model, save = ns["parse_model"](deepcopy(cfg), ch=[3])
    det = model[-1]
    det.stride = torch.tensor(spec.stride)              # Model.__init__ derives them from a 256 x 256 forward
    det.anchors /= det.stride.view(-1, 1, 1)
    for m in model.modules():                           # initialize_weights
        if type(m) is nn.BatchNorm2d:
            m.eps, m.momentum = 1e-3, 0.03
    wrapped = nn.Module()
    wrapped.model = model
    wrapped.load_state_dict(state_dict, strict=True)
    unfused = [(k, list(v.shape)) for k, v in wrapped.state_dict().items()]
    wrapped.eval()
    for m in model.modules():                           # Model.fuse
        if type(m) is ns["Conv"] and hasattr(m, "bn"):
            m.conv = ns["fuse_conv_and_bn"](m.conv, m.bn)
            delattr(m, "bn")
            m.forward = m.fuseforward
    fused = [(k, list(v.shape)) for k, v in wrapped.state_dict().items()]
    det.train()                                         # the training branch returns the conv outputs
    return model, save, unfused, fused


def forward_once(model, save, x):
    y, outs = [], []
    for m in model:
        if m.f != -1:
            x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
        if type(m).__name__ == "Detect":
            x = [m.m[i](v) for i, v in enumerate(x)]    # Detect.forward's first line per level (yolo.py:52)
        else:
            x = m(x)
        y.append(x if m.i in save else None)
        outs.append(x)
    return x, outs


def figures(got, want):
    return [T.rel_l2(got, want), T.worst(got, want)]


def main(ref):
    ns = reference_namespace(ref)
    arrays, out = {}, {"cases": {}, "leaves": {}, "keys": {}}
    for name, (narrow, bs, h, w, wseed, xseed) in T.CASES.items():
        cfg = T.load_cfg(narrow)
        spec, sd, x = T.case_inputs(name)
        model, save, unfused, fused = build_reference(ns, cfg, spec, sd)
        assert save == spec.save, (save, spec.save)
        out["keys"]["narrow" if narrow else "yolov5s"] = {"unfused": unfused, "fused": fused}
        with torch.no_grad():
            heads, layers = forward_once(model, save, torch.from_numpy(x))
        assert all(hd.dtype == torch.float32 for hd in heads)
        heads64, layers64 = T.network64(spec, sd, x)
        row = dict(narrow=narrow, bs=bs, h=h, w=w, weight_seed=wseed, input_seed=xseed,
                   sha256_input=T.sha256(x), sha256_weights=T.sha256(*[v.numpy() for v in sd.values()]),
                   parameters=int(sum(p.numel() for p in model.parameters())),
                   heads=[figures(g, t) for g, t in zip(heads, heads64)],
                   layers=[None if t is None else figures(g, t) for g, t in zip(layers[:-1], layers64[:-1])],
                   head_shapes=[list(hd.shape) for hd in heads])
        for l, hd in enumerate(heads):
            arrays["%s/head%d" % (name, l)] = hd.numpy()
        out["cases"][name] = row
        print(name, row["parameters"], ["%.2e" % f[0] for f in row["heads"]])
    for name, c in T.LEAVES.items():
        a = T.leaf_inputs(name)
        x = torch.from_numpy(a["x"])
        with torch.no_grad():
            if c.get("pool"):
                spp = ns["SPP"](2 * c["c1"], 8)
                got = torch.cat([m(x) for m in spp.m], 1)
            else:
                m = ns["Focus"](c["c1"] // 4, c["c2"], c["k"], c["s"]) if c.get("focus") else ns["Conv"](c["c1"], c["c2"], c["k"], c["s"])
                cv = m.conv if c.get("focus") else m
                cv.conv = nn.Conv2d(c["c1"], c["c2"], c["k"], c["s"], ns["autopad"](c["k"]), bias=True)
                cv.conv.weight.copy_(torch.from_numpy(a["w"]))
                cv.conv.bias.copy_(torch.from_numpy(a["b"]))
                cv.forward = cv.fuseforward
                got = m(x)
                if a["res"] is not None:
                    got = torch.from_numpy(a["res"]) + got          # Bottleneck.forward: x + cv2(...)
        arrays["leaf/" + name] = got.numpy()
        out["leaves"][name] = dict(shape=list(got.shape), sha256_input=T.sha256(*[v for v in a.values() if v is not None]))
        print(name, list(got.shape))
    out["source"] = ("autopad, Conv, Bottleneck, C3, SPP, Focus, Concat, Detect, parse_model, make_divisible and "
                     "fuse_conv_and_bn of the reference, cut with ast, on CPU torch %s" % torch.__version__.split("+")[0])
    with open(os.path.join(HERE, "ref_detector.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_detector.npz"), **arrays)
    print("wrote", len(arrays), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
