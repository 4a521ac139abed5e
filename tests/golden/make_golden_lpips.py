"""Generate tests/golden/ref_lpips.json.  Needs a checkout of the reference (GaussianRPG); never run by a test:

    python tests/golden/make_golden_lpips.py <path to the reference>

The reference's LPIPS imports torchvision (not installed here; its weights are a download), so the modules cannot be
imported.  This script cuts ``normalize_activation`` (lib/utils/lpipsPyTorch/modules/utils.py), ``get_network``,
``LinLayers``, ``BaseNet`` (with its ``z_score`` and ``forward``), ``AlexNet`` and ``VGG16`` (networks.py) and ``LPIPS``
(lpips.py) out of the reference with ``ast`` -- as the other makers do -- and runs them in float32 on CPU torch.  The
stand-ins cover only what those classes ask of the outside: ``models.alexnet(...)`` / ``models.vgg16(...)``, whose
``.features`` are ``nn.Sequential``s built from the tables of tests/lpips_truth.py with its seeded weights, and
``get_state_dict``, which returns the seeded ``lin`` weights under the renamed keys.  ``load_state_dict`` in
``LPIPS.__init__`` pins those key names and shapes.

The file holds numbers and names only.  Per case: the reference's [1, 1, 1, 1] result, the float64 truth's per-pair
values and tap terms, and the sha256 of the generated inputs.  Per net: the sha256 of the generated weights and, for
every tap, pooled over that net's cases, the reference's own relative L2 distance of its per-pixel maps
``l((fx - fy) ** 2)`` from the float64 truth and its mean absolute error -- what the acceptance bounds are made of.
"""
import ast
import json
import os
import sys
from collections import OrderedDict
from itertools import chain
from typing import Sequence

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lpips_truth as T          # noqa: E402

MODULES = "lib/utils/lpipsPyTorch/modules"
WANTED = {MODULES + "/utils.py": ("normalize_activation",),
          MODULES + "/networks.py": ("get_network", "LinLayers", "BaseNet", "AlexNet", "VGG16"),
          MODULES + "/lpips.py": ("LPIPS",)}


def sequential(net):
    """torchvision's ``features`` from the table, with the seeded weights."""
    mods, sd = [], T.build_features(net)
    for L in T.LAYERS[net]:
        if L[0] == "conv":
            mods.append(nn.Conv2d(L[1], L[2], L[3], L[4], L[5]))
        elif L[0] == "relu":
            mods.append(nn.ReLU(inplace=True))
        else:
            mods.append(nn.MaxPool2d(L[1], L[2]))
    seq = nn.Sequential(*mods)
    seq.load_state_dict(sd, strict=True)
    return seq


class _Models:
    class VGG16_Weights:
        IMAGENET1K_V1 = "IMAGENET1K_V1"

    @staticmethod
    def alexnet(*args, **kw):
        m = nn.Module()
        m.features = sequential("alex")
        return m

    @staticmethod
    def vgg16(*args, **kw):
        m = nn.Module()
        m.features = sequential("vgg")
        return m


def reference_namespace(ref):
    ns = {"torch": torch, "nn": nn, "chain": chain, "Sequence": Sequence, "OrderedDict": OrderedDict, "models": _Models,
          "get_state_dict": lambda net_type="alex", version="0.1": OrderedDict(T.renamed(T.build_lin(net_type)))}
    for rel, names in WANTED.items():
        path = os.path.join(ref, rel)
        with open(path) as f:
            tree = ast.parse(f.read())
        body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
        assert sorted(n.name for n in body) == sorted(names), (rel, [n.name for n in body])
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def main(ref):
    ns = reference_namespace(ref)
    out = {"cases": {}, "nets": {}}
    pooled = {net: [[] for _ in range(5)] for net in T.LAYERS}
    for net in T.LAYERS:
        crit = ns["LPIPS"](net)
        crit.eval()
        assert list(crit.net.target_layers) == list(T.TARGETS[net]) and list(crit.net.n_channels_list) == list(T.CHANNELS[net])
        for name, (cnet, pairs, h, w, seed) in T.CASES.items():
            if cnet != net:
                continue
            _, features, lin, x, y = T.case_inputs(name)
            tx, ty = torch.from_numpy(x), torch.from_numpy(y)
            with torch.no_grad():
                value = crit(tx, ty)
                assert value.dtype == torch.float32 and list(value.shape) == [1, 1, 1, 1]
                # the per-pixel maps of LPIPS.forward, before its mean: the reference's own modules
                diff = [(fx - fy) ** 2 for fx, fy in zip(crit.net(tx), crit.net(ty))]
                maps = [l(d)[:, 0] for d, l in zip(diff, crit.lin)]
            truth = T.truth64(net, features, lin, x, y)
            for l in range(5):
                assert maps[l].shape == truth["maps"][l].shape, (name, l, maps[l].shape, truth["maps"][l].shape)
                pooled[net][l].append((maps[l], truth["maps"][l]))
            out["cases"][name] = dict(net=net, pairs=pairs, h=h, w=w, input_seed=seed, sha256_input=T.sha256(x, y),
                                      reference=float(value), truth_total=truth["total"],
                                      truth_values=truth["values"].tolist(), truth_taps=truth["taps"].tolist(),
                                      tap_shapes=[list(m.shape[1:]) for m in truth["maps"]])
            print(name, float(value), truth["total"])
        figs = [T.pooled_map_figures(p) for p in pooled[net]]
        out["nets"][net] = dict(sha256_weights=T.weights_hash(net), map_rel_l2=[f[0] for f in figs],
                                map_mean_abs=[f[1] for f in figs])
        print(net, ["%.2e" % f[0] for f in figs], ["%.2e" % f[1] for f in figs])
    out["source"] = ("normalize_activation, get_network, LinLayers, BaseNet, AlexNet, VGG16 and LPIPS of the reference, cut "
                     "with ast, float32 on CPU torch %s" % torch.__version__.split("+")[0])
    with open(os.path.join(HERE, "ref_lpips.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
