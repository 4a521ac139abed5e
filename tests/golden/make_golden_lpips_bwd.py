"""Generate tests/golden/ref_lpips_bwd.json.  Needs a checkout of the reference (GaussianRPG); never run by a test:

    python tests/golden/make_golden_lpips_bwd.py <path to the reference>

As make_golden_lpips.py (whose stand-ins and ``ast`` cut this script reuses), it runs the reference's own
``lpipsPyTorch`` modules -- ``LPIPS`` over ``AlexNet`` / ``VGG16``, ``LinLayers`` and ``normalize_activation`` -- in
float32 on CPU torch with the seeded backbones, here WITH autograd on ``x``: the gradient of ``LPIPS.forward`` (the sum
over the pairs) over the six CASES of tests/lpips_truth.py.

The file holds numbers and names only.  Per case: the sha256 of the inputs and of the weights, and how far the
reference's own float32 gradient lies from the conditional float64 truth of tests/lpips_bwd_truth.py AT THE
REFERENCE'S OWN float32 DECISIONS (its post-ReLU activations, read with forward hooks: act > 0, and every pool's first
row-major maximum): the relative L2 distance and the worst element's distance -- what the acceptance bound of the
backward is made of -- with the truth's norm and largest magnitude for scale.
"""
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lpips_bwd_truth as B      # noqa: E402
import lpips_truth as T          # noqa: E402
import make_golden_lpips as G    # noqa: E402


def main(ref):
    ns = G.reference_namespace(ref)
    out = {"cases": {}}
    for net in T.LAYERS:
        crit = ns["LPIPS"](net)
        crit.eval()
        n_convs = sum(l["kind"] == "conv" for l in B.plan(net))
        kept = []
        for m in crit.net.layers:
            if isinstance(m, nn.ReLU):
                m.register_forward_hook(lambda mod, inp, outp: kept.append(outp.detach().clone()))
        for name, (cnet, pairs, h, w, seed) in T.CASES.items():
            if cnet != net:
                continue
            _, features, lin, x, y = T.case_inputs(name)
            tx, ty = torch.from_numpy(x).clone().requires_grad_(True), torch.from_numpy(y)
            del kept[:]
            value = crit(tx, ty)
            acts = kept[:n_convs]                                   # LPIPS.forward runs the net on x first
            assert [a.shape[0] for a in acts] == [pairs] * n_convs
            grad, = torch.autograd.grad(value.sum(), tx)
            assert grad.dtype == torch.float32 and grad.shape == tx.shape
            masks, winners = B.decisions_of(net, acts)
            truth = B.grad64(net, features, lin, x, y, masks=masks, winners=winners)
            rel, worst = B.figures(grad, truth)
            own = B.forward64(net, features, x)
            flips = sum(int((a != b).sum()) for a, b in zip(masks, own["masks"]))
            out["cases"][name] = dict(net=net, pairs=pairs, h=h, w=w, input_seed=seed, sha256_input=T.sha256(x, y),
                                      sha256_weights=T.weights_hash(net), rel_l2=rel, worst=worst,
                                      truth_norm=float(torch.linalg.norm(truth.reshape(-1))),
                                      truth_max=float(truth.abs().max()), relu_flips_vs_float64=flips)
            print(name, "rel L2 %.3e worst %.3e (truth max %.3e), ReLU decisions unlike float64's: %d"
                  % (rel, worst, float(truth.abs().max()), flips))
    out["source"] = ("LPIPS, AlexNet, VGG16, LinLayers and normalize_activation of the reference, cut with ast, float32 on "
                     "CPU torch %s with autograd on x" % torch.__version__.split("+")[0])
    with open(os.path.join(HERE, "ref_lpips_bwd.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
