"""Generate tests/golden/ref_ssim.npz from the reference's own loss code.  Run in the build container only:

    python tests/golden/make_golden_ssim.py <path of a GaussianRPG checkout>

lib/utils/loss_utils.py imports lib.config (and img_utils), which do not resolve outside the reference
tree, so -- as make_golden.py does for other modules -- the functions gaussian, create_window, ssim,
_ssim and l1_loss are cut out with ast and executed here, on CPU, in float64.  Recorded per case: the
inputs (and mask), SSIM with size_average True (and False for 4-D input), L1, and the float64 autograd
gradients of SSIM, L1 and the train.py:118 mix (lambda_dssim 0.2) with respect to img1.
The tests read only the .npz (tests/test_ssim_reference.py)."""
import ast
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def _extract_functions(path, names):
    src = open(path).read()
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), [f.name for f in fns]
    from torch.autograd import Variable
    ns = {"torch": torch, "F": F, "Variable": Variable, "exp": math.exp}
    exec(compile(ast.Module(fns, []), os.path.basename(path), "exec"), ns)
    return ns


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_ssim.py <path of a GaussianRPG checkout>")
    ns = _extract_functions(os.path.join(sys.argv[1], "lib/utils/loss_utils.py"),
                            ["gaussian", "create_window", "ssim", "_ssim", "l1_loss"])
    ref_ssim, ref_l1 = ns["ssim"], ns["l1_loss"]
    rng = np.random.RandomState(2024)
    cases = {
        # name: (shape, mask shape or None)
        "c13x17": ((3, 13, 17), None),
        "c37x53_mask": ((3, 37, 53), (1, 37, 53)),
        "c5x7": ((3, 5, 7), None),
        "c5x7_mask": ((3, 5, 7), (1, 5, 7)),
        "c1x1": ((3, 1, 1), None),
        "b2x3x20x30": ((2, 3, 20, 30), None),
        "b2x3x20x30_mask": ((2, 3, 20, 30), (2, 1, 20, 30)),
        "g1x16x24": ((1, 16, 24), None),
    }
    out = {"names": np.array(sorted(cases))}
    for name, (shape, mshape) in sorted(cases.items()):
        x1 = rng.rand(*shape)
        x2 = np.clip(x1 + 0.2 * rng.randn(*shape), 0, 1)
        out[name + "/img1"] = x1
        out[name + "/img2"] = x2
        mask = None
        if mshape is not None:
            mk = rng.rand(*mshape) > 0.3
            out[name + "/mask"] = mk
            mask = torch.from_numpy(mk)
        a = torch.from_numpy(x1)
        b = torch.from_numpy(x2)

        t = a.clone().requires_grad_(True)
        s = ref_ssim(t, b, mask=mask)
        s.backward()
        out[name + "/ssim"] = s.detach().numpy()
        out[name + "/grad_ssim"] = t.grad.numpy()
        if len(shape) == 4:
            out[name + "/ssim_per_image"] = ref_ssim(a, b, size_average=False, mask=mask).numpy()

        if len(shape) == 3:   # loss_utils.l1_loss takes (C,H,W) images and a (1,H,W) mask
            t = a.clone().requires_grad_(True)
            v = ref_l1(t, b, mask)
            v.backward()
            out[name + "/l1"] = v.detach().numpy()
            out[name + "/grad_l1"] = t.grad.numpy()
            t = a.clone().requires_grad_(True)
            lam = 0.2
            v = (1.0 - lam) * 1.0 * ref_l1(t, b, mask) + lam * (1.0 - ref_ssim(t, b, mask=mask))
            v.backward()
            out[name + "/mix"] = v.detach().numpy()
            out[name + "/grad_mix"] = t.grad.numpy()
    path = os.path.join(HERE, "ref_ssim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
