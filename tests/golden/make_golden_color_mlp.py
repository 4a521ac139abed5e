"""Generate tests/golden/ref_color_mlp.json + ref_color_mlp.npz.  Needs a checkout of the reference (GaussianRPG); never
run by a test:

    python tests/golden/make_golden_color_mlp.py <path to the reference>

Cuts ``get_affine_trans``, ``forward`` and ``regularization_loss`` out of the reference's lib/models/color_correction.py
and ``matrix_to_axis_angle``, ``matrix_to_quaternion``, ``_sqrt_positive_part`` and ``quaternion_to_axis_angle`` out of
its lib/utils/general_utils.py with ``ast`` (the modules themselves import the config, CUDA extensions and packages that
are not installed here) and executes them on CPU tensors over a stub object that holds what
``ColorCorrection.__init__`` sets up for the ``use_mlp`` variant (color_correction.py:10-13, 24-50: ``identity_matrix``,
``config.use_mlp = True``, the two ``nn.Sequential`` networks), one camera at a time.

The files hold numbers only.  Inputs are not stored: a case names its builders in tests/color_mlp_truth.py (legacy
numpy RandomState: stable) and records the sha256 of the input bytes.  Recorded per case, all float32: the 6-vector
``matrix_to_axis_angle`` returned, both matrices, ``regularization_loss``, and the autograd gradients at all sixteen
tensors of  sum(grad_affine[0,0] * A) + sum(grad_affine[0,1] * A_sky) + grad_reg[0] * regularization_loss  with the
named upstream gradients.  ``forward`` is executed on a small image and held against the recorded matrix here.
"""
import ast
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import color_mlp_truth as mt   # noqa: E402  (the input builders)

METHODS = ["get_affine_trans", "forward", "regularization_loss"]
FUNCTIONS = ["matrix_to_axis_angle", "matrix_to_quaternion", "_sqrt_positive_part", "quaternion_to_axis_angle"]


def _reference(ref):
    ns = {"torch": torch, "F": F, "Camera": object}
    path = os.path.join(ref, "lib", "utils", "general_utils.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCTIONS]
    assert sorted(n.name for n in funcs) == sorted(FUNCTIONS)
    exec(compile(ast.fix_missing_locations(ast.Module(body=funcs, type_ignores=[])), path, "exec"), ns)
    path = os.path.join(ref, "lib", "models", "color_correction.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ColorCorrection"][0]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in methods) == sorted(METHODS)
    stub = ast.ClassDef(name="ColorCorrectionMethods", bases=[], keywords=[], body=methods, decorator_list=[])
    exec(compile(ast.fix_missing_locations(ast.Module(body=[stub], type_ignores=[])), path, "exec"), ns)
    return ns


class _Config:
    use_mlp = True


class _Camera:
    def __init__(self, ego_pose, extrinsic):
        self.ego_pose, self.extrinsic = torch.from_numpy(ego_pose.copy()), torch.from_numpy(extrinsic.copy())
        self.id, self.meta = 0, dict(cam=0)


def _network(params, net):
    seq = nn.Sequential(nn.Linear(6, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(),
                        nn.Linear(64, 12))
    seq.load_state_dict({k[len(net) + 1:]: torch.from_numpy(v.copy()) for k, v in params.items()
                         if k.startswith(net + ".")})
    return seq


def _stub(ns, params):
    o = ns["ColorCorrectionMethods"]()
    o.identity_matrix = torch.eye(4).float()[:3]
    o.config = _Config()
    o.mode = "image"
    o.affine_trans = _network(params, "affine_trans")
    o.affine_trans_sky = _network(params, "affine_trans_sky")
    o.cur_affine_trans = None
    return o


def _cases():
    out = [dict(name=pose, pose=pose, seed=mt.SEED, zero_last=False) for pose in mt.POSES]
    out.append(dict(name="fresh_dominant_r", pose="dominant_r", seed=mt.SEED, zero_last=True))
    return out


def main(ref):
    ns = _reference(ref)
    arrays, rows = {}, []
    ga, gr = mt.build_grad_affine(1, seed=1), mt.build_grad_reg(1, seed=1)
    for c in _cases():
        params = mt.build_params(c["seed"], c["zero_last"])
        o = _stub(ns, params)
        ego, ext = mt.build_pose(c["pose"])
        camera = _Camera(ego, ext)
        x = ns["matrix_to_axis_angle"]((camera.ego_pose @ camera.extrinsic).unsqueeze(0)).squeeze(0)
        A = o.get_affine_trans(camera, use_sky=False)
        A_sky = o.get_affine_trans(camera, use_sky=True)
        reg = o.regularization_loss(camera)
        loss = (torch.from_numpy(ga[0, 0]) * A).sum() + (torch.from_numpy(ga[0, 1]) * A_sky).sum() + float(gr[0]) * reg
        loss.backward()
        image = torch.rand(3, 2, 3, generator=torch.Generator().manual_seed(0))
        for use_sky, M in ((False, A), (True, A_sky)):
            want = torch.einsum("ij,jhw->ihw", M[:, :3], image) + M[:, 3, None, None]
            assert torch.equal(o.forward(camera, image, use_sky=use_sky), want)
        rec = dict(x=x.detach().numpy(), affine=torch.stack([A, A_sky]).detach().numpy(),
                   reg=reg.detach().numpy().reshape(1))
        sd = dict(("affine_trans." + k, v) for k, v in o.affine_trans.named_parameters())
        sd.update(("affine_trans_sky." + k, v) for k, v in o.affine_trans_sky.named_parameters())
        assert sorted(sd) == sorted(mt.KEYS)
        for k in mt.KEYS:
            rec["grad/" + k] = sd[k].grad.numpy().copy()
        for k, v in rec.items():
            assert v.dtype == np.float32 and np.all(np.isfinite(v)), (c["name"], k)
            arrays["%s/%s" % (c["name"], k)] = v
        rows.append(dict(c, grad_affine=dict(T=1, seed=1), grad_reg=dict(T=1, seed=1),
                         sha256=mt.sha256(ego, ext, ga, gr, *[params[k] for k in mt.KEYS])))
        print("%-22s x %s" % (c["name"], np.array2string(rec["x"], precision=5)))
    source = ("lib/models/color_correction.py (%s) and lib/utils/general_utils.py (%s) of the reference, cut with ast "
              "and executed on CPU torch %s over a stub of the use_mlp variant"
              % (", ".join(METHODS), ", ".join(FUNCTIONS), torch.__version__.split("+")[0]))
    with open(os.path.join(HERE, "ref_color_mlp.json"), "w") as f:
        json.dump({"source": source, "cases": rows}, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "ref_color_mlp.npz"), **arrays)
    print("wrote %d cases, %d arrays" % (len(rows), len(arrays)))


if __name__ == "__main__":
    main(sys.argv[1])
