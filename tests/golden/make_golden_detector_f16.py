"""Generate tests/golden/ref_detector_f16.json.  Needs a checkout of the reference (GaussianRPG); never run by a test:

    python tests/golden/make_golden_detector_f16.py <path to the reference>

Works as make_golden_detector.py does and uses its functions: the reference's modules are cut with ``ast`` at run time
from the reference tree, ``parse_model`` builds the network, the seeded weights of tests/detector_truth.py are loaded
and every ``Conv`` fused the way ``Model.fuse`` does.  Then the model is put in half, as the reference's detectors run
it (``model.half()``; its checkpoints are stored in half), and walked on CPU torch with the input ``.half()``.

Per whole-network case and head: the relative L2 distance and the worst element distance of the reference's half heads
from the float64 truth over the unfused float32 state dict (detector_truth.network64), and the head shapes.  Results
only: numbers and names."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_detector as G    # noqa: E402  (puts tests/ and the repository on the path)
import detector_truth as T          # noqa: E402


def main(ref):
    ns = G.reference_namespace(ref)
    out = {"cases": {}}
    for name, (narrow, bs, h, w, wseed, xseed) in T.CASES.items():
        spec, sd, x = T.case_inputs(name)
        model, save, _, _ = G.build_reference(ns, T.load_cfg(narrow), spec, sd)
        model.half()
        with torch.no_grad():
            heads, _ = G.forward_once(model, save, torch.from_numpy(x).half())
        assert all(hd.dtype == torch.float16 for hd in heads)
        heads64, _ = T.network64(spec, sd, x)
        out["cases"][name] = dict(narrow=narrow, bs=bs, h=h, w=w, weight_seed=wseed, input_seed=xseed,
                                  sha256_input=T.sha256(x), sha256_weights=T.sha256(*[v.numpy() for v in sd.values()]),
                                  heads=[G.figures(g.float(), t) for g, t in zip(heads, heads64)],
                                  head_shapes=[list(hd.shape) for hd in heads])
        print(name, ["%.2e" % f[0] for f in out["cases"][name]["heads"]])
    out["source"] = ("the modules make_golden_detector.py cuts from the reference, fused, .half(), input .half(), on CPU "
                     "torch %s" % torch.__version__.split("+")[0])
    with open(os.path.join(HERE, "ref_detector_f16.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
